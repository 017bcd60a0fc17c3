"""Autograd shim of the fused InstanceNorm3d(affine)+ReLU kernels
(include/transoar_instnorm.h) for channels-last bf16 activations."""
import torch

from . import _native
from ._native import launch
from .conv3d import to_ndhwc

lib = _native.bind("instnorm", abi=3)
CL3D = torch.channels_last_3d


def supported(x, channels):
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 5 and channels % 8 == 0
            and 192 % (channels // 8) == 0)


class _InstNormReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, part=None):
        x = to_ndhwc(x)
        n, c = x.shape[:2]
        v = x.shape[2] * x.shape[3] * x.shape[4]
        y = torch.empty_like(x, memory_format=CL3D)
        g32, b32 = gamma.float().contiguous(), beta.float().contiguous()
        ws = torch.empty((n, c, 2), dtype=torch.float64, device=x.device)
        mean_rstd = torch.empty((n, c, 2), dtype=torch.float32, device=x.device)
        if part is not None:
            # the statistics were taken in the epilogue of the convolution that produced x (conv3d.Conv3dK3.forward_with_stats)
            launch(lib.transoar_instnorm_relu_forward_parts, x, x.data_ptr(), g32.data_ptr(), b32.data_ptr(), y.data_ptr(),
                   part.data_ptr(), part.shape[0] // n, ws.data_ptr(), mean_rstd.data_ptr(),
                   n, v, c, float(eps), 1 if relu else 0)
        else:
            launch(lib.transoar_instnorm_relu_forward, x, x.data_ptr(), g32.data_ptr(), b32.data_ptr(), y.data_ptr(),
                   ws.data_ptr(), mean_rstd.data_ptr(), n, v, c, float(eps), 1 if relu else 0)
        ctx.save_for_backward(x, g32, b32, mean_rstd)
        ctx.relu, ctx.param_dtype = relu, gamma.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g32, b32, mean_rstd = ctx.saved_tensors
        dy = to_ndhwc(dy)
        n, c = x.shape[:2]
        v = x.shape[2] * x.shape[3] * x.shape[4]
        dx = torch.empty_like(x, memory_format=CL3D)
        red = torch.empty((n, c, 2), dtype=torch.float64, device=x.device)
        dparams = torch.empty((2, c), dtype=torch.float32, device=x.device)      # dbeta | dgamma, summed over the samples by the kernel
        launch(lib.transoar_instnorm_relu_backward, x, x.data_ptr(), dy.data_ptr(), g32.data_ptr(), b32.data_ptr(),
               mean_rstd.data_ptr(), dx.data_ptr(), red.data_ptr(), dparams.data_ptr(), n, v, c, 1 if ctx.relu else 0)
        return dx, dparams[1].to(ctx.param_dtype), dparams[0].to(ctx.param_dtype), None, None, None


def instance_norm_relu(x, gamma, beta, eps=1e-5, relu=True, part=None):
    """relu(instance_norm(x) * gamma + beta) for (N,C,D,H,W) bf16 on the GPU.  part: the per-workgroup partial sums of x's
    statistics when the producing convolution took them in its epilogue (conv3d.Conv3dK3.forward_with_stats)."""
    return _InstNormReLU.apply(x, gamma, beta, eps, relu, part)
