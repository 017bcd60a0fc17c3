"""GPU: one case per route of conv_plan.plan_conv, at the smallest shape that reaches it.  Conv3dK3 must issue exactly the
launches the plan names, in its order, and y, dx, dW, db must match PyTorch's fp32 convolution on the same bf16-rounded
inputs.  Tolerances are those of tests/test_conv3d_gpu.py: bf16 outputs 2^-7 of the tensor's max, fp32 weight and bias
gradients 2e-3."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [  # (N, Cin, Cout, D, H, W, stride), with statistics, (fwd, dgrad, wgrad) it must reach
    ((2, 24, 24, 3, 4, 64, 1), False, ("direct", "direct_flipped", "lds_tr")),
    ((1, 1, 24, 18, 30, 128, 1), False, ("c1_halo", None, "c1_tr")),
    ((1, 1, 8, 2, 3, 48, 1), False, ("c1_padded", None, "c1")),
    ((1, 24, 24, 18, 22, 200, 1), True, ("stats_halo", "direct_flipped", "voxel_major")),
    ((1, 96, 96, 5, 5, 8, 1), False, ("igemm", "igemm_s1", "voxel_major")),              # split-K both ways
    ((1, 48, 48, 24, 32, 64, 1), False, ("igemm", "igemm_s1", "voxel_major")),           # no split
    ((1, 24, 48, 8, 8, 16, 2), False, ("igemm", "s2_halo", "voxel_major")),
    ((2, 48, 96, 4, 6, 16, 2), False, ("igemm", "s2_classes", "voxel_major")),
    ((1, 48, 48, 16, 256, 64, 1), False, ("igemm", "igemm_s1", "ring")),                 # 2^18 rows
    # 2^21 rows: two batch ranges each way and the LDS weight gradient in four 32-channel blocks.  (The same row count in
    # ONE sample, (1, 48, 48, 128, 256, 64, 1), is refused by the implicit-GEMM forward: tests/test_conv_plan.py.)
    ((2, 48, 48, 128, 128, 64, 1), False, ("igemm", "igemm_s1", "lds_tr")),
    ((1, 1, 40, 2, 3, 16, 1), False, ("c1_padded", None, "channels_first")),
]


def relerr(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("shape,stats,routes", CASES, ids=["x".join(map(str, c[0])) + ("-stats" if c[1] else "") for c in CASES])
def test_conv_runs_the_planned_launches(shape, stats, routes, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transoar_amd import conv3d, conv_gemm
    from transoar_amd.conv_plan import plan_conv
    n, ci, co, d, h, w, s = shape
    plan = plan_conv(*shape, stats)
    assert (plan.fwd, plan.dgrad if ci != 1 else None, plan.wgrad) == routes
    if routes[2] == "lds_tr" and co > 32:
        assert len(plan.wgrad_blocks) == 4 and len(plan.fwd_ranges) == 2

    seen = []
    real = conv3d.launch

    def recording(fn, *args, **kwargs):
        seen.append(fn.__name__)
        return real(fn, *args, **kwargs)

    monkeypatch.setattr(conv3d, "launch", recording)
    monkeypatch.setattr(conv_gemm, "launch", recording)
    monkeypatch.setattr(conv3d.Conv3dK3, "min_voxels", 0)

    torch.manual_seed(ci * 1000 + co)
    conv = conv3d.Conv3dK3(ci, co, 3, stride=s, padding=1, bias=True).cuda()
    x = torch.randn(n, ci, d, h, w, device="cuda").to(torch.bfloat16)
    if ci != 1:
        x = x.contiguous(memory_format=torch.channels_last_3d).requires_grad_()
    if stats:
        y, part = conv.forward_with_stats(x)
        assert part is not None and tuple(part.shape) == (plan.stat_rows, 2, 32)
    else:
        y = conv(x)
    assert seen == plan.launches("fwd")
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last_3d)

    xr = x.detach().float().requires_grad_(ci != 1)
    wr = conv.weight.detach().to(torch.bfloat16).float().requires_grad_()
    br = conv.bias.detach().float().clone().requires_grad_()
    yr = F.conv3d(xr, wr, br, stride=s, padding=1)
    assert tuple(y.shape) == tuple(yr.shape)
    assert relerr(y, yr) <= 2.0 ** -7

    g = torch.randn_like(yr).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)
    del seen[:]
    y.backward(g)
    assert seen == (plan.launches("dgrad") if ci != 1 else []) + plan.launches("wgrad")
    yr.backward(g.float())
    assert relerr(conv.weight.grad, wr.grad) <= 2e-3
    assert relerr(conv.bias.grad, br.grad) <= 2e-3
    if ci != 1:
        assert relerr(x.grad, xr.grad) <= 2.0 ** -7
