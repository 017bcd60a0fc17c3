#!/usr/bin/env python
"""Dense head-dimension-48 cross-attention (csrc/dense_attn.hip) against the torch route it replaces in
FocusedAttn.forward (transposed head views + F.scaled_dot_product_attention with the additive (Nq, L) mask), on the same
device and inputs, at the two shipped configs' shapes: B = 2, H = 8, (Nq, L) = (405, 16 384) and (1 080, 12 800); without a
mask (restrict_attn False) and with per-organ windows of 60 % of the keys (boxes too large to gather).  The two routes
are timed alternately; one JSON line per (shape, mask, route) on stdout and in --out."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transoar_amd import dense_attn  # noqa: E402

H, HD = 8, 48


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "dense_attn_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    lines = []
    for b, n_q, n_keys, n_org in ((2, 405, 16384, 15), (2, 1080, 12800, 20)):
        g = torch.Generator().manual_seed(n_q)
        q, k, v, d_o = (torch.randn(b, n, H * HD, generator=g).to(torch.bfloat16).cuda() for n in (n_q, n_keys, n_keys, n_q))
        q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
        for mask_name in ("none", "windows"):
            mask = torch.zeros(n_q, n_keys, dtype=torch.bool)
            if mask_name == "windows":
                rows, width = n_q // n_org, int(0.6 * n_keys)
                for o in range(n_org):
                    lo = (n_keys - width) * o // (n_org - 1)
                    mask[o * rows:(o + 1) * rows, :lo] = True
                    mask[o * rows:(o + 1) * rows, lo + width:] = True
            mask = mask.cuda()
            bits = dense_attn.key_bits(mask, n_org)
            bias = None if bits is None else torch.zeros(n_q, n_keys, device="cuda").masked_fill_(mask, float("-inf")).to(torch.bfloat16)

            def fused():
                return dense_attn.dense_attention(q, k, v, bits, HD ** -0.5)

            def torch_route():
                heads = lambda t: t.view(b, -1, H, HD).transpose(1, 2)          # noqa: E731
                x = F.scaled_dot_product_attention(heads(q), heads(k), heads(v), attn_mask=bias, scale=HD ** -0.5)
                return x.transpose(1, 2).reshape(b, n_q, H * HD)

            def both_ways(fn):
                def run():
                    q.grad = k.grad = v.grad = None
                    fn().backward(d_o)
                return run

            with torch.no_grad():
                err = float((fused().float() - torch_route().float()).abs().max())
            routes = (("fused", fused), ("torch_sdpa", torch_route))
            for _ in range(3):                                   # warm up every shape and direction of both routes
                for _, fn in routes:
                    fn()
                    both_ways(fn)()
            res = {name: {"fwd": [], "fwd_bwd": []} for name, _ in routes}
            for _ in range(3):                                   # alternate the routes: the host is shared
                for name, fn in routes:
                    res[name]["fwd"].append(time_ms(fn, args.iters))
                    res[name]["fwd_bwd"].append(time_ms(both_ways(fn), args.iters))
            for name, _ in routes:
                f_ms, fb_ms = (sorted(res[name][key])[1] for key in ("fwd", "fwd_bwd"))
                lines.append({"op": "dense_attention", "impl": name, "B": b, "H": H, "Nq": n_q, "L": n_keys, "mask": mask_name,
                              "fwd_ms": round(f_ms, 4), "fwd_bwd_ms": round(fb_ms, 4),
                              "fwd_spread_ms": round(max(res[name]["fwd"]) - min(res[name]["fwd"]), 4),
                              "max_abs_diff_between_routes": round(err, 5)})
                print(json.dumps(lines[-1]), flush=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
