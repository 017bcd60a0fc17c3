#!/usr/bin/env python
"""Detection targets from the flagship's label volume (2 x 1 x 160 x 160 x 256, 20 organs painted from synthetic boxes), uint8 and
int64: the kernel pair of csrc/box_targets.hip against the batched torch restatement (box_targets.targets_from_labels_torch) on
the device, hipEvents around N calls after a warm-up.  Bytes/s are against the label bytes, read once.

    python tools/bench_box_targets.py [--warmup 20] [--reps 200] [--cpu-reps 3] [--out FILE.jsonl]

--cpu-reps > 0 also times the torch restatement on CPU tensors (what a data loader on this host would pay per batch)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests._seg_inputs import paint_labels  # noqa: E402
from transoar_amd import box_targets  # noqa: E402
from transoar_amd.config import synthetic_targets  # noqa: E402

N, K, SHAPE = 2, 20, (160, 160, 256)


def us_per_call(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    host = paint_labels(synthetic_targets(N, K, seed=1), SHAPE)
    rows = []
    for dtype in (torch.uint8, torch.int64):
        labels = host.to(dtype).cuda()
        boxes = torch.empty(N, K, 6, device="cuda")
        present = torch.empty(N, K, dtype=torch.bool, device="cuda")
        counts = torch.empty(2, device="cuda")
        ws = torch.empty(box_targets.workspace_bytes(N, labels[0].numel(), K) // 4, dtype=torch.int32, device="cuda")
        ref = box_targets.targets_from_labels_torch(labels, K, 1)
        box_targets.box_targets_into(labels, K, 1, 5, boxes, present, counts, ws)
        assert torch.equal(boxes, ref.boxes) and torch.equal(present, ref.present) and float(counts[0]) == float(ref.num_boxes)
        hip = us_per_call(lambda: box_targets.box_targets_into(labels, K, 1, 5, boxes, present, counts, ws), args.warmup, args.reps)
        tor = us_per_call(lambda: box_targets.targets_from_labels_torch(labels, K, 1), args.warmup, args.reps)
        byt = labels.numel() * labels.element_size()
        row = {"labels": str(dtype)[6:], "shape": [N, 1] + list(SHAPE), "classes": K, "boxes_found": int(ref.present.sum()),
               "reps": args.reps, "hip_us": round(hip, 2), "torch_device_us": round(tor, 1), "speedup": round(tor / hip, 1),
               "label_MB": round(byt / 1e6, 1), "hip_bytes_per_s": round(byt / (hip * 1e-6)),
               "fraction_of_6.29TBps_copy": round(byt / (hip * 1e-6) / 6.29e12, 3)}
        if args.cpu_reps > 0:
            cpu = host.to(dtype)
            box_targets.targets_from_labels_torch(cpu, K, 1)
            t0 = time.perf_counter()
            for _ in range(args.cpu_reps):
                box_targets.targets_from_labels_torch(cpu, K, 1)
            row.update(torch_cpu_us=round((time.perf_counter() - t0) * 1e6 / args.cpu_reps), cpu_threads=torch.get_num_threads())
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
