"""ConvPatchMerging on the patch_merge kernels + fused InstanceNorm/ReLU, under bf16 autocast, against a deep copy of the
module in fp64 on the CPU (the stock nn.Sequential route).

Bounds (max|a - b| / max|b| per tensor): twice what the stock route (TRANSOAR_PATCH_MERGE_FUSED=0: MIOpen conv + torch
InstanceNorm3d + ReLU under the same autocast) measured in this very comparison on an MI355X, DESIGN.md section 12.15:
out 0.00608, d_x 0.0509, d_conv_weight 0.1523, d_norm_weight 0.01514, d_norm_bias 0.0822.  With 54 voxels per channel the
gradients' error is that of single ReLU decisions that bf16 flips next to zero, on either route."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
BOUNDS = {"out": 0.0121, "d_x": 0.1017, "d_conv_weight": 0.3046, "d_norm_weight": 0.0302, "d_norm_bias": 0.1644}


def _inputs():
    g = torch.Generator().manual_seed(48)
    x = torch.randn(2, 4, 6, 6, 48, generator=g).to(torch.bfloat16)
    d_out = torch.randn(2, 2, 3, 3, 96, generator=g).to(torch.bfloat16)
    return x, d_out, torch.rand(96, generator=g) + 0.5, torch.randn(96, generator=g) * 0.2


def _grads(module, x, d_out):
    x = x.clone().requires_grad_(True)
    out = module(x)
    out.backward(d_out.to(out.dtype))
    conv, norm = module._reduction[0], module._reduction[1]
    return {"out": out.detach(), "d_x": x.grad, "d_conv_weight": conv.weight.grad, "d_norm_weight": norm.weight.grad,
            "d_norm_bias": norm.bias.grad}


def test_module_matches_fp64_and_takes_the_fused_route(monkeypatch):
    from transoar_amd import patch_merge
    from transoar_amd.swin_encoder import ConvPatchMerging
    torch.manual_seed(0)
    module = ConvPatchMerging(dim=48)
    x, d_out, gamma, beta = _inputs()
    with torch.no_grad():
        module._reduction[1].weight.copy_(gamma)
        module._reduction[1].bias.copy_(beta)
    assert sorted(module.state_dict()) == ["_reduction.0.weight", "_reduction.1.bias", "_reduction.1.weight"]
    ref = _grads(copy.deepcopy(module).double(), x.double(), d_out.double())

    calls, apply = [], patch_merge.PatchMergeConv.apply
    monkeypatch.setattr(patch_merge.PatchMergeConv, "apply", staticmethod(lambda *a: calls.append(1) or apply(*a)))
    module = module.cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = _grads(module, x.cuda(), d_out.cuda())
    errs = {k: float((got[k].double().cpu() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}
    print("fused" if calls else "stock", errs)
    assert len(calls) == 1
    assert got["out"].shape == (2, 2, 3, 3, 96) and got["d_conv_weight"].dtype == torch.float32
    for k, bound in BOUNDS.items():
        assert errs[k] <= bound, (k, errs[k], bound)
