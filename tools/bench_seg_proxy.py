#!/usr/bin/env python
"""The segmentation proxy's head and losses at the flagship's P0 (2 x 24 x 160 x 160 x 256, bf16 channels-last), K = 2 and 21:
the torch path (nn.Conv3d on MIOpen; TransoarCriterion.loss_segmentation's softmax / one-hot / tp-fp-fn tensors under bf16
autocast) against the kernels of csrc/seg_proxy.hip, forward and backward, timed with hipEvents (median of N).  GB/s are
against algorithmic bytes: every input read once and every output written once (bf16 maps, 1-byte labels).

    python tools/bench_seg_proxy.py [--reps N] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys

os.environ.setdefault("MIOPEN_USER_DB_PATH", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "miopen_db"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transoar_amd import seg_proxy  # noqa: E402
from transoar_amd.criterion import TransoarCriterion  # noqa: E402

N, C, SHAPE = 2, 24, (160, 160, 256)
CL = torch.channels_last_3d


def t_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))[reps // 2]


def mirror(logits, labels, fg_bg):
    crit = TransoarCriterion(20, None, seg_proxy=True, seg_fg_bg=fg_bg)
    was, seg_proxy.ENABLED = seg_proxy.ENABLED, False
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return crit.loss_segmentation({"pred_seg": logits}, labels)
    finally:
        seg_proxy.ENABLED = was


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    v = N * SHAPE[0] * SHAPE[1] * SHAPE[2]
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((N, C) + SHAPE, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_()
    labels = torch.randint(0, 21, (N, 1) + SHAPE, device="cuda", generator=g).to(torch.uint8)
    rows = []
    for k, fg_bg in ((2, True), (21, False)):
        conv = torch.nn.Conv3d(C, k, kernel_size=1).cuda()
        dy = torch.randn((N, k) + SHAPE, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
        logits = (2 * torch.randn((N, k) + SHAPE, device="cuda", generator=g)).to(torch.bfloat16).contiguous(memory_format=CL)
        logits.requires_grad_()
        byt = {"head_fwd": v * (2 * C + 2 * k), "head_bwd": v * (2 * C + 2 * k + 2 * C),
               "loss_fwd": v * (2 * k + 1), "loss_bwd": v * (2 * k + 1 + 2 * k)}

        def hip_head_fwd():
            with torch.no_grad():
                seg_proxy.seg_head(x, conv)

        def torch_head_fwd():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                conv(x)

        y_hip = seg_proxy.seg_head(x, conv)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y_t = conv(x)
        hip = {"head_fwd": t_ms(hip_head_fwd, args.reps),
               "head_bwd": t_ms(lambda: torch.autograd.grad(y_hip, (x, conv.weight, conv.bias), dy, retain_graph=True), args.reps)}
        tor = {"head_fwd": t_ms(torch_head_fwd, args.reps),
               "head_bwd": t_ms(lambda: torch.autograd.grad(y_t, (x, conv.weight, conv.bias), dy, retain_graph=True), args.reps)}
        vec = seg_proxy.seg_loss_vector(logits, labels, fg_bg)
        tot = 2 * vec[0] + 2 * vec[1]
        hip["loss_fwd"] = t_ms(lambda: seg_proxy.seg_loss_vector(logits.detach(), labels, fg_bg), args.reps)
        hip["loss_bwd"] = t_ms(lambda: torch.autograd.grad(tot, logits, retain_graph=True), args.reps)
        ce, dice = mirror(logits, labels, fg_bg)
        tot_t = 2 * ce + 2 * dice

        def torch_loss_fwd():
            with torch.no_grad():
                mirror(logits.detach(), labels, fg_bg)
        tor["loss_fwd"] = t_ms(torch_loss_fwd, max(3, args.reps // 4))
        tor["loss_bwd"] = t_ms(lambda: torch.autograd.grad(tot_t, logits, retain_graph=True), max(3, args.reps // 4))
        del y_hip, y_t, vec, tot, ce, dice, tot_t
        for name in ("head_fwd", "head_bwd", "loss_fwd", "loss_bwd"):
            row = {"K": k, "op": name, "hip_ms": round(hip[name], 4), "torch_ms": round(tor[name], 4),
                   "speedup": round(tor[name] / hip[name], 1), "alg_MB": round(byt[name] / 1e6, 1),
                   "hip_GBps": round(byt[name] / hip[name] / 1e6, 0), "floor_ms_6.3TBps": round(byt[name] / 6.3e9, 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    for k in (2, 21):
        h = sum(r["hip_ms"] for r in rows if r["K"] == k)
        t = sum(r["torch_ms"] for r in rows if r["K"] == k)
        rows.append({"K": k, "op": "total", "hip_ms": round(h, 4), "torch_ms": round(t, 4), "speedup": round(t / h, 1)})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
