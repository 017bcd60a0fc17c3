"""Convolutional patch merging (csrc/patch_merge.hip through include/transoar_patchmerge.h) against F.conv3d in fp64 on the
CPU with the bf16-rounded x, weight and dy permuted to NCDHW.  Bounds, tensor-max normalised: 2^-7 on the bf16 y and dx (the
bf16-storage rule), 1e-4 on the fp32 dW."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, 2, 2, 16), (2, 5, 6, 7, 48), (1, 4, 6, 70, 32), (2, 2, 4, 4, 96), (1, 2, 2, 4, 768)]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """-> (x bf16, weight fp32 holding bf16 values, dy bf16) on the GPU and the fp64 reference (y, dx, dW), computed once."""
    b, d, h, w, c = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(torch.bfloat16)
    weight = (torch.randn(2 * c, c, 2, 2, 2, generator=g) * (8 * c) ** -0.5).to(torch.bfloat16).float()
    dy = torch.randn(b, d // 2, h // 2, w // 2, 2 * c, generator=g).to(torch.bfloat16)
    x64, w64 = x.double().requires_grad_(True), weight.double().requires_grad_(True)
    y = F.conv3d(x64.permute(0, 4, 1, 2, 3), w64, stride=2).permute(0, 2, 3, 4, 1)
    y.backward(dy.double())
    return (x.cuda(), weight.cuda(), dy.cuda()), (y.detach(), x64.grad, w64.grad)


def _run(shape):
    from transoar_amd import patch_merge
    x, weight, dy = (t.clone() for t in _case(shape)[0])
    x.requires_grad_(True), weight.requires_grad_(True)
    y = patch_merge.patch_merge_conv(x, weight)
    y.backward(dy)
    return y.detach(), x.grad, weight.grad


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("shape", SHAPES)
def test_patch_merge_matches_fp64(shape):
    y, dx, dw = _run(shape)
    ref_y, ref_dx, ref_dw = _case(shape)[1]
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16 and dw.dtype == torch.float32
    errs = {"y": _rel(y, ref_y), "dx": _rel(dx, ref_dx), "dW": _rel(dw, ref_dw)}
    print(shape, errs)
    assert errs["y"] <= 2 ** -7 and errs["dx"] <= 2 ** -7 and errs["dW"] <= 1e-4, errs
    assert torch.equal(dw, _run(shape)[2])                               # fixed summation order: bit-equal from run to run


def test_dropped_voxels_get_exact_zeros():
    dx = _run((2, 5, 6, 7, 48))[1]
    assert bool((dx[:, 4] == 0).all()) and bool((dx[:, :, :, 6] == 0).all())
    assert bool((dx[:, :4, :, :6] != 0).any())


@pytest.mark.parametrize("what", ["channels", "bias"])
def test_refusals(what):
    from transoar_amd import patch_merge
    c = 24 if what == "channels" else 32
    conv = torch.nn.Conv3d(c, 2 * c, 2, 2, bias=what == "bias").cuda()
    x = torch.zeros(1, 2, 2, 2, c, dtype=torch.bfloat16, device="cuda")
    assert not patch_merge.usable(x, conv)
    if what == "channels":                                               # the raw call: its negative code, nothing launched
        y = torch.zeros(1, 1, 1, 1, 2 * c, dtype=torch.bfloat16, device="cuda")
        rc = patch_merge.lib.transoar_patch_merge_forward(x.data_ptr(), y.data_ptr(), y.data_ptr(), None, 0, 1, 2, 2, 2, c, None)
        assert rc == -2
        assert patch_merge.lib.transoar_patch_merge_pack(conv.weight.data_ptr(), 0, y.data_ptr(), c, None) == -2
