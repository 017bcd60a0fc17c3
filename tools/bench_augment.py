#!/usr/bin/env python
"""Batch augmentation at the flagship batch (2 x 1 x 160 x 160 x 256, uint8 and int32 labels): the one launch of csrc/augment.hip
against the batched torch restatement (augment.augment_torch) on the device, alternating in rounds, hipEvents around the calls of
a round after a warm-up.  Two tables: a shipped-style one (rotation, zoom, translation, gain, offset: eight corners per output)
and the identity (one corner per output: what the validation split costs).  Bytes/s are against the algorithmic bytes -- image
and labels read once and written once, (4 + sizeof(label)) * 2 per voxel -- and are also given as a share of a plain device copy
of the same number of bytes timed in the same run.

    python tools/bench_augment.py [--warmup 20] [--reps 200] [--torch-reps 10] [--rounds 3] [--out profiles/augment_bench.jsonl]

The reference's host chain (MONAI) is not installed and is not measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transoar_amd import augment  # noqa: E402

N, SHAPE = 2, (160, 160, 256)
A_MIN, A_MAX = 0.1, 0.9


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


def tables():
    shipped = augment.compose_params(N, SHAPE, angles=[[4.3, -3.1, 4.9], [-4.3, 3.1, -4.9]], zoom=[1.07, 0.93],
                                     translate=[[-11.0, 9.0, -19.0], [11.0, -9.0, 19.0]], gain=[1.07, 0.95], offset=[-0.04, 0.06])
    return {"shipped": shipped, "identity": augment.compose_params(N, SHAPE)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment.py measures on the GPU; there is no CPU figure"
    g = torch.Generator().manual_seed(0)
    image = torch.rand(N, 1, *SHAPE, generator=g).cuda()
    host_labels = torch.randint(0, 21, (N, 1, *SHAPE), generator=g)
    rows = []
    for dtype in (torch.uint8, torch.int32):
        labels = host_labels.to(dtype).cuda()
        out = (torch.empty_like(image), torch.empty_like(labels))
        byt = 2 * image.numel() * (4 + labels.element_size())
        src, dst = torch.empty(byt // 2, dtype=torch.uint8, device="cuda"), torch.empty(byt // 2, dtype=torch.uint8, device="cuda")
        for tag, host_table in tables().items():
            table = host_table.cuda()
            assert augment.usable(image, labels)
            ref, ref_lab = augment.augment_torch(image, labels, table, SHAPE, A_MIN, A_MAX, dtype=torch.float64)
            augment.augment_into(image, labels, table, out[0], out[1], A_MIN, A_MAX)
            err = float((out[0].double() - ref).abs().max() / ref.abs().max())
            lab_diff = float((out[1] != ref_lab).double().mean())
            assert err <= 1e-4 and lab_diff <= 1e-3, (err, lab_diff)
            del ref, ref_lab
            hip, tor, cpy = [], [], []
            for _ in range(args.rounds):                      # alternating: kernel, restatement, copy
                hip.append(us_per_call(lambda: augment.augment_into(image, labels, table, out[0], out[1], A_MIN, A_MAX),
                                       args.warmup, args.reps))
                tor.append(us_per_call(lambda: augment.augment_torch(image, labels, table, SHAPE, A_MIN, A_MAX), 2, args.torch_reps))
                cpy.append(us_per_call(lambda: dst.copy_(src), args.warmup, args.reps))
            best, copy = min(hip), min(cpy)
            row = {"labels": str(dtype)[6:], "table": tag, "shape": [N, 1] + list(SHAPE), "reps": args.reps, "rounds": args.rounds,
                   "hip_us": [round(t, 2) for t in hip], "torch_device_us": [round(t, 1) for t in tor],
                   "copy_us": [round(t, 2) for t in cpy], "speedup_over_torch": round(min(tor) / best, 1),
                   "algorithmic_MB": round(byt / 1e6, 1), "hip_bytes_per_s": round(byt / (best * 1e-6)),
                   "copy_bytes_per_s": round(byt / (copy * 1e-6)), "share_of_measured_copy": round(copy / best, 3),
                   "share_of_6.29TBps_copy": round(byt / (best * 1e-6) / 6.29e12, 3),
                   "max_err_vs_fp64": err, "labels_differing": lab_diff, "reference_host_chain": "not measured"}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
