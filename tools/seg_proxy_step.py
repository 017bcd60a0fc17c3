#!/usr/bin/env python
"""Milliseconds per training step of the flagship (VISCERAL 160 x 160 x 256, batch 2, refine on, bf16) with the segmentation proxy
loss on (fg_bg: K = 2, the shipped setting) and off, eager and captured (one HIP graph per step), hipEvents over the timed steps
after a warm-up, on the capture stream as bench.py runs them.

    python tools/seg_proxy_step.py [--steps N] [--warmup W] [--modes off-eager,off-graph,on-eager,on-graph] [--out FILE.json]

Under `rocprofv3 --kernel-trace --stats` with --modes on-eager,on-graph it shows which kernels a seg-proxy step launches (no
MIOpen convolution)."""
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


def run(seg, graph, steps, warmup):
    cfg = visceral_config(refine=True, use_cuda=True)
    cfg["backbone"]["use_seg_proxy_loss"] = seg
    cfg["bbox_properties"] = synthetic_bbox_properties(20, seed=0)
    torch.manual_seed(0)
    model = TransoarNet(cfg).cuda()
    step = TrainStep(model, build_criterion(cfg), cfg, amp_dtype=torch.bfloat16, graph=graph)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand(2, 1, 160, 160, 256, device="cuda", generator=g)
    targets = synthetic_targets(2, 20, seed=1, device="cuda")
    tg = DenseTargets.from_list(targets, 20, "cuda")
    labels = paint_labels(targets, (160, 160, 256)).to(torch.uint8).cuda() if seg else None
    side = step.capture_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if graph:
            step.capture(x, tg, labels)
        for _ in range(warmup):
            total, losses = step(x, tg, labels)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            total, losses = step(x, tg, labels)
        end.record()
    torch.cuda.synchronize()
    out = {"seg_proxy": seg, "graph": graph, "steps": steps, "ms_per_step": round(start.elapsed_time(end) / steps, 3),
           "total": round(float(total), 4)}
    if seg:
        out.update(segce=round(float(losses["segce"]), 5), segdice=round(float(losses["segdice"]), 5))
    del step, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--modes", default="off-eager,off-graph,on-eager,on-graph")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for mode in args.modes.split(","):
        seg, kind = mode.split("-")
        rows.append(run(seg == "on", kind == "graph", args.steps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
