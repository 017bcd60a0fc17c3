#!/usr/bin/env python
"""The case resize (csrc/resize.hip) at its two callers' sizes, against the same operation in torch on the device
(F.interpolate mode='area' on the image and mode='nearest' on the labels of the slice), alternating in rounds, hipEvents around the
calls of a round after a warm-up.

  preparation  a raw-sized case 1 x 512 x 512 x 400, int16 image and uint8 labels, the window from foreground_window on a
               synthetic body mask, -> (160, 160, 256): foreground window (two launches) + resize (one launch)
  test split   2 x 1 x 200 x 180 x 300 fp32 (uint8 labels), range scaling, -> the median (160, 160, 256): one launch

Bytes/s are against the algorithmic bytes -- the window's voxels read once (image and labels; for the preparation also the
whole label map once, for the window) and the outputs written once -- and are also given as a share of a plain device copy of the
same number of bytes timed in the same run.

    python tools/bench_resize.py [--warmup 20] [--reps 200] [--torch-reps 20] [--rounds 3] [--out profiles/resize_bench.jsonl]

The reference's host chain (MONAI) is not installed and is not measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from transoar_amd import resize  # noqa: E402

TARGET = (160, 160, 256)
A_MIN, A_MAX = -57.0, 164.0


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


def body_mask(shape):
    """A synthetic body: an ellipsoid of label 1 with a few organs (2..6) inside, off-centre, well inside the volume."""
    d, h, w = (torch.arange(s, dtype=torch.float32) for s in shape)
    r = ((d[:, None, None] - 0.52 * shape[0]) / (0.40 * shape[0])) ** 2 + ((h[None, :, None] - 0.47 * shape[1]) / (0.33 * shape[1])) ** 2 \
        + ((w[None, None, :] - 0.50 * shape[2]) / (0.45 * shape[2])) ** 2
    lab = (r < 1).to(torch.uint8)
    for c in range(2, 7):
        lo = [int(s * (0.25 + 0.06 * c)) for s in shape]
        lab[lo[0]:lo[0] + shape[0] // 10, lo[1]:lo[1] + shape[1] // 10, lo[2]:lo[2] + shape[2] // 10] = c
    return lab[None]


def torch_resize(image, labels, window, a_min=None, a_max=None):
    """The same operation in torch on the device: slice each sample's window (a host table), F.interpolate."""
    xs, ls = [], []
    for s, row in enumerate(window):
        sl = tuple(slice(row[a], row[a] + row[3 + a]) for a in range(3))
        v = image[s][sl][None, None].float()
        if a_min is not None:
            v = ((v - a_min) / (a_max - a_min)).clamp(0, 1)
        xs.append(F.interpolate(v, size=TARGET, mode="area"))
        ls.append(F.interpolate(labels[s][sl][None, None].float(), size=TARGET, mode="nearest").to(labels.dtype))
    return torch.cat(xs), torch.cat(ls)


def measure(tag, ours, theirs, byt, args, extra):
    src, dst = torch.empty(byt // 2, dtype=torch.uint8, device="cuda"), torch.empty(byt // 2, dtype=torch.uint8, device="cuda")
    hip, tor, cpy = [], [], []
    for _ in range(args.rounds):                      # alternating: kernels, torch on the device, copy
        hip.append(us_per_call(ours, args.warmup, args.reps))
        tor.append(us_per_call(theirs, 2, args.torch_reps))
        cpy.append(us_per_call(lambda: dst.copy_(src), args.warmup, args.reps))
    best, copy = min(hip), min(cpy)
    row = {"row": tag, "reps": args.reps, "rounds": args.rounds, "hip_us": [round(t, 2) for t in hip],
           "torch_device_us": [round(t, 1) for t in tor], "copy_us": [round(t, 2) for t in cpy],
           "speedup_over_torch": round(min(tor) / best, 1), "algorithmic_MB": round(byt / 1e6, 1),
           "hip_bytes_per_s": round(byt / (best * 1e-6)), "copy_bytes_per_s": round(byt / (copy * 1e-6)),
           "share_of_measured_copy": round(copy / best, 3), "reference_host_chain": "not measured"}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resize.py measures on the GPU; there is no CPU figure"
    g = torch.Generator().manual_seed(0)
    rows = []

    # ---- preparation: foreground window + resize of a raw-sized case
    shape = (512, 512, 400)
    labels = body_mask(shape).cuda()
    image = torch.randint(-1024, 3072, (1, *shape), generator=g, dtype=torch.int16).cuda()
    assert resize.usable(image, labels)
    window = torch.empty(1, resize.WINDOW, dtype=torch.int32, device="cuda")
    ws = torch.empty(resize.workspace_bytes(1, labels[0].numel()) // 4, dtype=torch.int32, device="cuda")
    out = (torch.empty(1, *TARGET, device="cuda"), torch.empty(1, *TARGET, dtype=torch.uint8, device="cuda"))

    def prepare():
        resize.foreground_window_into(labels, window, ws, None, 5)
        resize.resize_into(image, labels, window, TARGET, out[0], out[1])

    prepare()
    host_window = window.cpu().tolist()
    ref, ref_lab = torch_resize(image, labels, host_window)
    err = float((out[0].double() - ref.view_as(out[0]).double()).abs().max() / ref.double().abs().max())
    lab_diff = float((out[1] != ref_lab.view_as(out[1])).double().mean())
    assert err <= 1e-4 and lab_diff == 0.0, (err, lab_diff)
    voxels = host_window[0][3] * host_window[0][4] * host_window[0][5]
    outs = TARGET[0] * TARGET[1] * TARGET[2]
    byt = labels.numel() + voxels * 3 + outs * 5          # the label map once for the window; the window's int16 + uint8; fp32 + uint8 out
    rows.append(measure("preparation", prepare, lambda: torch_resize(image, labels, host_window), byt, args,
                        {"shape": [1] + list(shape), "image": "int16", "labels": "uint8", "window": host_window[0][:6],
                         "target": list(TARGET), "launches": 3, "max_err_vs_torch": err, "labels_differing": lab_diff}))
    only = us_per_call(lambda: resize.resize_into(image, labels, window, TARGET, out[0], out[1]), args.warmup, args.reps)
    rows[-1]["resize_launch_alone_us"] = round(only, 2)
    rows[-1]["resize_alone_bytes_per_s"] = round((voxels * 3 + outs * 5) / (only * 1e-6))
    del image, labels, ref, ref_lab

    # ---- the test split: range scaling, area / nearest to the median
    shape = (200, 180, 300)
    image = torch.rand(2, 1, *shape, generator=g).mul_(400).sub_(150).cuda()
    labels = torch.randint(0, 21, (2, 1, *shape), generator=g).to(torch.uint8).cuda()
    assert resize.usable(image, labels)
    out = (torch.empty(2, 1, *TARGET, device="cuda"), torch.empty(2, 1, *TARGET, dtype=torch.uint8, device="cuda"))
    table = resize.whole_window(2, shape).cuda()

    def split():
        resize.resize_into(image, labels, table, TARGET, out[0], out[1], A_MIN, A_MAX)

    split()
    host_window = table.cpu().tolist()
    ref, ref_lab = torch_resize(image[:, 0], labels[:, 0], host_window, A_MIN, A_MAX)
    err = float((out[0].double() - ref.double()).abs().max() / ref.double().abs().max())
    lab_diff = float((out[1] != ref_lab).double().mean())
    assert err <= 1e-4 and lab_diff == 0.0, (err, lab_diff)
    byt = image.numel() * 5 + 2 * outs * 5
    rows.append(measure("test_split", split, lambda: torch_resize(image[:, 0], labels[:, 0], host_window, A_MIN, A_MAX), byt, args,
                        {"shape": [2, 1] + list(shape), "image": "float32", "labels": "uint8", "target": list(TARGET), "launches": 1,
                         "max_err_vs_torch": err, "labels_differing": lab_diff}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
