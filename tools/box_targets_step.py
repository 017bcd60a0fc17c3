#!/usr/bin/env python
"""Milliseconds per captured training step of the flagship (VISCERAL 160 x 160 x 256, batch 2, refine on, bf16) with the box targets
given (DenseTargets computed once, outside the timing) and with targets=None (the box-target launches are the first nodes of the
graph), in one process, hipEvents over the timed steps after a warm-up, on the capture stream as bench.py runs them.  Every mode
builds its own model and graph, as tools/seg_proxy_step.py does; the modes are run alternately so that the run-to-run spread
shows next to the difference.

    python tools/box_targets_step.py [--steps 50] [--warmup 10] [--seg-proxy] [--modes given,labels,given,labels] [--out FILE.json]"""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests._seg_inputs import paint_labels  # noqa: E402
from transoar_amd.config import synthetic_bbox_properties, synthetic_targets, visceral_config  # noqa: E402
from transoar_amd.matcher import DenseTargets  # noqa: E402
from transoar_amd.train_step import TrainStep  # noqa: E402
from transoar_amd.transoarnet import TransoarNet, build_criterion  # noqa: E402


def run(from_labels, seg, steps, warmup):
    cfg = visceral_config(refine=True, use_cuda=True)
    cfg["backbone"]["use_seg_proxy_loss"] = seg
    cfg["bbox_properties"] = synthetic_bbox_properties(20, seed=0)
    torch.manual_seed(0)
    model = TransoarNet(cfg).cuda()
    step = TrainStep(model, build_criterion(cfg), cfg, amp_dtype=torch.bfloat16, graph=True)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand(2, 1, 160, 160, 256, device="cuda", generator=g)
    labels = paint_labels(synthetic_targets(2, 20, seed=1), (160, 160, 256)).to(torch.uint8).cuda()
    tg = None if from_labels else DenseTargets.from_labels(labels, 20, cfg["bbox_padding"])
    seg_targets = labels if (seg or from_labels) else None
    side = step.capture_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step.capture(x, tg, seg_targets)
        for _ in range(warmup):
            total, losses = step(x, tg, seg_targets)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            total, losses = step(x, tg, seg_targets)
        end.record()
    torch.cuda.synchronize()
    out = {"targets": "from_labels_in_graph" if from_labels else "given", "seg_proxy": seg, "steps": steps,
           "ms_per_step": round(start.elapsed_time(end) / steps, 3), "total": round(float(total), 4)}
    del step, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seg-proxy", action="store_true")
    ap.add_argument("--modes", default="given,labels,given,labels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for mode in args.modes.split(","):
        rows.append(run(mode == "labels", args.seg_proxy, args.steps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    given = [r["ms_per_step"] for r in rows if r["targets"] == "given"]
    lab = [r["ms_per_step"] for r in rows if r["targets"] != "given"]
    if given and lab:
        rows.append({"labels_minus_given_ms": round(sum(lab) / len(lab) - sum(given) / len(given), 3),
                     "given_ms": given, "from_labels_ms": lab})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
