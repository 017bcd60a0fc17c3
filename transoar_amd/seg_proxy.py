"""The segmentation proxy loss (backbone.use_seg_proxy_loss) on hand-written kernels (include/transoar_segproxy.h,
csrc/seg_proxy.hip): the 1x1x1 segmentation head on the full-resolution FPN level P0 (transoar/models/transoarnet.py:38-42,
121,138) and the softmax cross-entropy + batch soft-Dice losses of transoar/models/criterion.py:77-90,127-197, each one
autograd Function over a forward and a backward launch pair.

The head and the losses stay two calls: `pred_seg` is a real tensor in the model's output dict (callers and the reference
expect it there), and the losses are the criterion's.  The torch code they replace (nn.Conv3d, which MIOpen runs, and
TransoarCriterion.loss_segmentation's softmax / one-hot / tp-fp-fn tensors at full resolution) stays the path for CPU
tensors, shapes the kernels do not take, and TRANSOAR_SEG_PROXY_HIP=0; it is what the GPU tests compare these kernels with.
"""
import os

import torch

from . import _native
from ._native import launch, ptr

lib = _native.bind("segproxy", abi=1)
ENABLED = os.environ.get("TRANSOAR_SEG_PROXY_HIP", "1") != "0"
MAX_C, MAX_K = 64, 32
NCDHW, NDHWC = 0, 1
_DT = {torch.float32: 0, torch.bfloat16: 2}
_LABEL_DT = {torch.uint8: 16, torch.int16: 17, torch.int32: 18, torch.int64: 19}


def _layout(t):
    """-> (layout code, t): contiguous NCDHW or channels-last NDHWC as it is, anything else made channels-last."""
    if t.is_contiguous():
        return NCDHW, t
    if not t.is_contiguous(memory_format=torch.channels_last_3d):
        t = t.contiguous(memory_format=torch.channels_last_3d)
    return NDHWC, t


def _workspace(c, k, dev):
    return torch.empty(lib.transoar_seg_workspace_bytes(c, k) // 4, dtype=torch.float32, device=dev)


# ---- head -------------------------------------------------------------------------------------------------------------------
def head_usable(x, conv):
    """Can the head kernels take Conv3d `conv` (kernel 1, with bias) on the map x?"""
    return (ENABLED and torch.is_tensor(x) and x.is_cuda and x.dim() == 5 and x.dtype in _DT
            and 1 <= conv.in_channels <= MAX_C and 1 <= conv.out_channels <= MAX_K and x.shape[1] == conv.in_channels
            and tuple(conv.kernel_size) == (1, 1, 1) and tuple(conv.stride) == (1, 1, 1) and tuple(conv.padding) == (0, 0, 0)
            and tuple(conv.dilation) == (1, 1, 1) and conv.groups == 1 and conv.bias is not None
            and conv.weight.is_cuda and conv.weight.device == x.device and conv.padding_mode == "zeros")


class _SegHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        xl, x = _layout(x)
        n, c, d, h, w = x.shape
        k = weight.shape[0]
        w32 = weight.detach().reshape(k, c).float().contiguous()
        b32 = bias.detach().float().contiguous()
        y = torch.empty((n, k, d, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last_3d)
        launch(lib.transoar_seg_head_forward, x, x.data_ptr(), xl, _DT[x.dtype], w32.data_ptr(), b32.data_ptr(), n, d * h * w, c, k,
               y.data_ptr())
        ctx.save_for_backward(x, w32)
        ctx.meta = (xl, weight.shape, weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32 = ctx.saved_tensors
        xl, wshape, wdt, bdt = ctx.meta
        n, c, d, h, w = x.shape
        k = w32.shape[0]
        dyl, dy = _layout(dy.to(x.dtype))
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None       # same layout as x
        dw = torch.empty(k, c, dtype=torch.float32, device=x.device)
        db = torch.empty(k, dtype=torch.float32, device=x.device)
        ws = _workspace(c, k, x.device)
        launch(lib.transoar_seg_head_backward, x, x.data_ptr(), xl, _DT[x.dtype], dy.data_ptr(), dyl, w32.data_ptr(), n, d * h * w, c, k,
               ptr(dx), dw.data_ptr(), db.data_ptr(), ws.data_ptr())
        return dx, dw.view(wshape).to(wdt), db.to(bdt)


def seg_head(x, conv):
    """conv(x) for the 1x1x1 segmentation head `conv` (an nn.Conv3d: its parameters and state-dict keys stay), on the head
    kernels: fp32 accumulation, the output channels-last in x's dtype."""
    return _SegHead.apply(x, conv.weight, conv.bias)


# ---- losses -----------------------------------------------------------------------------------------------------------------
def losses_usable(pred_seg, seg_targets):
    """Can the loss kernels take these logits (N, K, D, H, W) and labels (N, 1, D, H, W) or (N, D, H, W)?"""
    if not (ENABLED and torch.is_tensor(pred_seg) and torch.is_tensor(seg_targets) and pred_seg.is_cuda
            and seg_targets.device == pred_seg.device and pred_seg.dim() == 5 and pred_seg.dtype in _DT
            and seg_targets.dtype in _LABEL_DT and 2 <= pred_seg.shape[1] <= MAX_K):
        return False
    n, spatial = pred_seg.shape[0], tuple(pred_seg.shape[2:])
    return tuple(seg_targets.shape) in ((n, 1) + spatial, (n,) + spatial)


class _SegLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, fg_bg, smooth_nom, smooth_denom):
        ll, logits = _layout(logits)
        n, k = logits.shape[0], logits.shape[1]
        s = logits[0, 0].numel()
        labels = labels.contiguous()
        losses = torch.empty(2, dtype=torch.float32, device=logits.device)
        stats = torch.empty(2 * k, dtype=torch.float32, device=logits.device)
        ws = _workspace(0, k, logits.device)
        launch(lib.transoar_seg_loss_forward, logits, logits.data_ptr(), ll, _DT[logits.dtype], labels.data_ptr(),
               _LABEL_DT[labels.dtype], n, s, k, int(bool(fg_bg)), float(smooth_nom), float(smooth_denom), losses.data_ptr(),
               stats.data_ptr(), ws.data_ptr())
        ctx.save_for_backward(logits, labels, stats)
        ctx.meta = (ll, bool(fg_bg))
        ctx.mark_non_differentiable(stats)
        return losses

    @staticmethod
    def backward(ctx, g):
        logits, labels, stats = ctx.saved_tensors
        ll, fg_bg = ctx.meta
        n, k = logits.shape[0], logits.shape[1]
        g = g.contiguous().float()          # the two upstream gradients stay on the device (a graph tensor in the captured step)
        grad = torch.empty_like(logits)     # same layout as the logits
        launch(lib.transoar_seg_loss_backward, logits, logits.data_ptr(), ll, _DT[logits.dtype], labels.data_ptr(),
               _LABEL_DT[labels.dtype], n, logits[0, 0].numel(), k, int(fg_bg), stats.data_ptr(), g.data_ptr(), grad.data_ptr())
        return grad, None, None, None, None


def seg_loss_vector(pred_seg, seg_targets, fg_bg, smooth_nom=1e-5, smooth_denom=1e-5):
    """-> fp32 tensor [segce, segdice] (differentiable in pred_seg).  The labels are read, never modified (under fg_bg the
    kernel maps label > 0 to 1 as it reads; the reference rewrites the caller's tensor, criterion.py:81-82)."""
    return _SegLosses.apply(pred_seg, seg_targets, fg_bg, smooth_nom, smooth_denom)


def seg_losses(pred_seg, seg_targets, fg_bg, smooth_nom=1e-5, smooth_denom=1e-5):
    """-> (segce, segdice), as TransoarCriterion.loss_segmentation."""
    return tuple(seg_loss_vector(pred_seg, seg_targets, fg_bg, smooth_nom, smooth_denom).unbind(0))
