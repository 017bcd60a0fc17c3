#!/usr/bin/env python
"""The intensity tail of the batch augmentation at the flagship batch (2 x 1 x 160 x 160 x 256 fp32): the kernel sequence of
csrc/augment.hip (transoar_augment_intensity) against its torch restatement (augment.intensity_torch) on the same device and a
plain device copy of the same bytes, alternating in rounds, hipEvents around the calls of a round after a warm-up.  Three
tables: noise only, smoothing only with sigma = 1 (radius 4), and all three steps with gain and offset.  Bytes are the
algorithmic ones: the image read once and written once (2 x 4 bytes per voxel), whatever the number of passes.

    python tools/bench_augment_intensity.py [--warmup 10] [--reps 100] [--torch-reps 3] [--rounds 3]
                                            [--out profiles/augment_intensity_bench.jsonl]

The reference's host chain (MONAI) is not installed and cannot be measured here."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tools.bench_augment import N, SHAPE, us_per_call  # noqa: E402
from transoar_amd import augment  # noqa: E402

NOISE, SMOOTH, CONTRAST = augment.NOISE, augment.SMOOTH, augment.CONTRAST


def tables():
    keys = [[0x1234, 0x5678], [0x9ABC, 0xDEF0]]
    return {
        "noise": (NOISE, augment.compose_intensity(N, flags=NOISE, noise_std=[0.05, 0.08], keys=keys)),
        "smooth_sigma1": (SMOOTH, augment.compose_intensity(N, flags=SMOOTH, sigma=[1.0, 1.0, 1.0])),
        "all": (NOISE | SMOOTH | CONTRAST, augment.compose_intensity(N, flags=NOISE | SMOOTH | CONTRAST, noise_std=[0.05, 0.08],
                                                                     sigma=[[0.5, 1.0, 0.8], [1.0, 0.6, 0.7]], gain=[1.05, 0.95],
                                                                     offset=-0.1, gamma=[0.7, 1.5], keys=keys)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment_intensity.py measures on the GPU; there is no CPU figure"
    image = torch.rand(N, 1, *SHAPE, generator=torch.Generator().manual_seed(0)).cuda()
    out, scratch, workspace = torch.empty_like(image), torch.empty_like(image), augment.intensity_workspace(N, image.device)
    byt = 2 * image.numel() * 4
    src, dst = torch.empty(byt // 2, dtype=torch.uint8, device="cuda"), torch.empty(byt // 2, dtype=torch.uint8, device="cuda")
    rows = []
    for tag, (steps, host_table) in tables().items():
        table = host_table.cuda()
        ref = augment.intensity_torch(image, table, dtype=torch.float64)
        augment.intensity_into(image, out, table, steps, scratch, workspace)
        err = float((out.double() - ref).abs().max() / ref.abs().max())
        assert err <= 1e-4, (tag, err)
        del ref
        hip, tor, cpy = [], [], []
        for _ in range(args.rounds):                          # alternating: kernels, restatement, copy
            hip.append(us_per_call(lambda: augment.intensity_into(image, out, table, steps, scratch, workspace), args.warmup, args.reps))
            tor.append(us_per_call(lambda: augment.intensity_torch(image, table), 1, args.torch_reps))
            cpy.append(us_per_call(lambda: dst.copy_(src), args.warmup, args.reps))
        best, copy = min(hip), min(cpy)
        row = {"table": tag, "steps": steps, "shape": [N, 1] + list(SHAPE), "reps": args.reps, "rounds": args.rounds,
               "hip_us": [round(t, 2) for t in hip], "torch_device_us": [round(t, 1) for t in tor], "copy_us": [round(t, 2) for t in cpy],
               "speedup_over_torch": round(min(tor) / best, 1), "algorithmic_MB": round(byt / 1e6, 1),
               "hip_bytes_per_s": round(byt / (best * 1e-6)), "share_of_measured_copy": round(copy / best, 3),
               "max_err_vs_fp64": err, "reference_host_chain": "not measured"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
