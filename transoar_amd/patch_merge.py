"""ctypes binding and autograd shim of the convolutional patch merging kernels (C ABI: include/transoar_patchmerge.h;
kernels: csrc/patch_merge.hip).

Reference semantics: the convolution of ConvPatchMerging (encoder_blocks.py), nn.Conv3d(C, 2C, kernel_size=2, stride=2,
padding=0, bias=False), taken on the (B, D, H, W, C) token map as it lies:

    y[b, d', h', w', :] = sum_{kd, kh, kw} W[:, :, kd, kh, kw] x[b, 2 d' + kd, 2 h' + kh, 2 w' + kw, :]

Forward, data gradient and weight gradient are bf16 MFMA kernels with fp32 accumulation; the weight gradient comes out in
fp32 in the parameter's layout and is bit-stable.  No fallback: the library must be built.
"""
import os

import torch

from . import _native
from ._native import launch

ABI_VERSION = 1
lib = _native.bind("patchmerge", abi=ABI_VERSION)
ENABLED = os.environ.get("TRANSOAR_PATCH_MERGE_FUSED", "1") != "0"
_DTYPE_CODE = {torch.float32: _native.F32, torch.bfloat16: _native.BF16}


def usable(x, conv):
    """Can the kernels take this merge?  x (B, D, H, W, C) bf16, dense, on the GPU; conv the module's k = s = 2 Conv3d
    without a bias; C a multiple of 16; the map below 2^31 bytes."""
    return (ENABLED and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 5 and x.is_contiguous()
            and conv.bias is None and x.shape[-1] % 16 == 0 and 16 <= x.shape[-1] < 8192
            and tuple(conv.weight.shape) == (2 * x.shape[-1], x.shape[-1], 2, 2, 2) and conv.weight.dtype in _DTYPE_CODE
            and tuple(conv.stride) == (2, 2, 2) and tuple(conv.padding) == (0, 0, 0) and conv.groups == 1
            and x.shape[0] >= 1 and min(x.shape[1:4]) >= 2 and x.numel() * 2 < (1 << 31))


def _workspace(what, shape, device):
    n_bytes = lib.transoar_patch_merge_workspace_bytes(what, *shape)
    return torch.empty(n_bytes, dtype=torch.uint8, device=device), n_bytes


class PatchMergeConv(torch.autograd.Function):
    """y (B, D/2, H/2, W/2, 2C) bf16 = the k = s = 2 convolution of x (B, D, H, W, C) bf16 with weight (2C, C, 2, 2, 2).
    weight is the fp32 parameter (the gradient's owner); mirror its bf16 copy inside a training step, or None."""

    @staticmethod
    def forward(ctx, x, weight, mirror):
        b, d, h, w, c = x.shape
        src = (weight if mirror is None else mirror).detach().contiguous()
        packed = torch.empty((2 * c, 8 * c), dtype=torch.bfloat16, device=x.device)
        launch(lib.transoar_patch_merge_pack, x, src.data_ptr(), _DTYPE_CODE[src.dtype], packed.data_ptr(), c)
        y = torch.empty((b, d // 2, h // 2, w // 2, 2 * c), dtype=torch.bfloat16, device=x.device)
        ws, ws_bytes = _workspace(0, x.shape, x.device)
        launch(lib.transoar_patch_merge_forward, x, x.data_ptr(), packed.data_ptr(), y.data_ptr(), ws.data_ptr(), ws_bytes,
               b, d, h, w, c)
        ctx.save_for_backward(x, packed)
        ctx.weight_dtype = weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, packed = ctx.saved_tensors
        b, d, h, w, c = x.shape
        dy = dy.to(torch.bfloat16).contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            launch(lib.transoar_patch_merge_dgrad, x, dy.data_ptr(), packed.data_ptr(), dx.data_ptr(), b, d, h, w, c)
        if ctx.needs_input_grad[1]:
            dw = torch.empty((2 * c, c, 2, 2, 2), dtype=torch.float32, device=x.device)
            ws, ws_bytes = _workspace(1, x.shape, x.device)
            launch(lib.transoar_patch_merge_wgrad, x, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws_bytes,
                   b, d, h, w, c)
            dw = dw.to(ctx.weight_dtype)
        return dx, dw, None


def patch_merge_conv(x, weight, mirror=None):
    return PatchMergeConv.apply(x, weight, mirror)
