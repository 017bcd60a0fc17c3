#!/usr/bin/env python
"""The k = s = 2 patch-merging convolution (csrc/patch_merge.hip) against the stock route it replaces in
ConvPatchMerging (nn.Conv3d through MIOpen on the permuted view, under bf16 autocast), on the same device and inputs, at the
four stage shapes of a flagship Swin configuration, B = 2: C = 96 / 192 / 384 / 768 on grids 80x80x128 ... 10x10x16.
The stock route is given the find-db the project ships (tools/miopen_db, through MIOPEN_USER_DB_PATH).  The two routes are
timed alternately in three rounds of --iters calls after warm-up; one JSON line per (shape, route) on stdout and in --out:
the median call of the median round, forward alone and forward + backward.  A stock call slower than 100 ms gets fewer
calls per round (the line says how many)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MIOPEN_USER_DB_PATH", os.path.join(ROOT, "tools", "miopen_db"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, ROOT)
from transoar_amd import patch_merge  # noqa: E402

STAGES = ((2, 80, 80, 128, 96), (2, 40, 40, 64, 192), (2, 20, 20, 32, 384), (2, 10, 10, 16, 768))


def time_ms(fn, iters):
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_merge_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    lines = []
    for shape in STAGES:
        b, d, h, w, c = shape
        g = torch.Generator().manual_seed(c)
        x = torch.randn(shape, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
        weight = (torch.randn(2 * c, c, 2, 2, 2, generator=g) * (8 * c) ** -0.5).cuda().requires_grad_(True)
        d_y = torch.randn(b, d // 2, h // 2, w // 2, 2 * c, generator=g).to(torch.bfloat16).cuda()

        def fused():
            return patch_merge.patch_merge_conv(x, weight)

        def stock():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return F.conv3d(x.permute(0, 4, 1, 2, 3), weight, stride=2).permute(0, 2, 3, 4, 1)

        def both_ways(fn):
            def run():
                x.grad = weight.grad = None
                fn().backward(d_y)
            return run

        with torch.no_grad():
            err = float((fused().float() - stock().float()).abs().max())
        routes = (("fused", fused), ("miopen", stock))
        for _ in range(3):
            for _, fn in routes:
                fn()
                both_ways(fn)()
        iters = {name: args.iters if time_ms(both_ways(fn), 1) < 100.0 else 5 for name, fn in routes}
        res = {name: {"fwd": [], "fwd_bwd": []} for name, _ in routes}
        for _ in range(3):                                   # alternate the routes: the host is shared
            for name, fn in routes:
                res[name]["fwd"].append(time_ms(fn, iters[name]))
                res[name]["fwd_bwd"].append(time_ms(both_ways(fn), iters[name]))
        for name, _ in routes:
            f_ms, fb_ms = (sorted(res[name][key])[1] for key in ("fwd", "fwd_bwd"))
            lines.append({"op": "patch_merge_conv", "impl": name, "B": b, "grid": [d, h, w], "C": c, "iters": iters[name],
                          "fwd_ms": round(f_ms, 4), "fwd_bwd_ms": round(fb_ms, 4),
                          "fwd_spread_ms": round(max(res[name]["fwd"]) - min(res[name]["fwd"]), 4),
                          "fwd_bwd_spread_ms": round(max(res[name]["fwd_bwd"]) - min(res[name]["fwd_bwd"]), 4),
                          "max_abs_diff_between_routes": round(err, 5)})
            print(json.dumps(lines[-1]), flush=True)
        del x, weight, d_y
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
