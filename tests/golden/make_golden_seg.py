#!/usr/bin/env python
"""Generate tests/golden/g12_seg_proxy.npz (the segmentation proxy loss) by IMPORTING THE REFERENCE, as make_golden.py does
for g1..g11: runs only where the reference is available, on the CPU; the GPU box only sees the .npz.

  (a) loss level, fp64: the reference's TransoarCriterion.loss_segmentation (transoar/models/criterion.py:77-90,127-197) on
      small random logits and labels (tests/_seg_inputs.py::LOSS_CASES): segce, segdice and the logits' gradient of
      a * segce + b * segdice.  The logits are stored in fp32 (the reference computes in fp64 on exactly those values), the
      gradient rounded to fp32.
  (b) whole model, eval mode: the small-width VISCERAL-geometry model of g7 with use_seg_proxy_loss=True, batch 1, on
      the analytic volume, with a label volume painted from the synthetic boxes (tests/_seg_inputs.py::paint_labels), for
      fg_bg on (K = 2) and off (K = 21): every loss, the weighted total, the gradients of _seg_head.weight / bias and of the
      P0 output convolution, and pred_seg at fixed positions.  Computed in fp64: the bias gradient of the head is a sum of
      13.1 M / 2 cancelling terms, and the reference's own fp32 run is 2.5 % (K = 2) and 7 % (K = 21) away from its fp64 value
      -- a fixture for the kernels, which sum it in fp32 per workgroup and fp64 across, has to be exact there.

    python tests/golden/make_golden_seg.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)


def _reference_model_imports():
    """The two container-only shims of make_golden.py (a stub timm.models.layers, Tensor.cuda = identity)."""
    import types
    import torch.nn as nn

    class _DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()

        def forward(self, x):
            return x
    tl = types.ModuleType("timm.models.layers")
    tl.trunc_normal_ = nn.init.trunc_normal_
    tl.DropPath = _DropPath
    sys.modules.update({"timm": types.ModuleType("timm"), "timm.models": types.ModuleType("timm.models"),
                        "timm.models.layers": tl})
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self


def loss_level(store):
    from tests._seg_inputs import LOSS_CASES, LOSS_GRAD_COEFS, loss_case_inputs
    from transoar.models.criterion import TransoarCriterion
    a, b = LOSS_GRAD_COEFS
    for tag, k, fg_bg, shape, label_range, absent, seed in LOSS_CASES:
        logits, labels = loss_case_inputs(k, shape, label_range, absent, seed)
        crit = TransoarCriterion(num_classes=20, matcher=None, seg_proxy=True, seg_fg_bg=fg_bg)
        x = logits.double().requires_grad_()
        ce, dice = crit.loss_segmentation({"pred_seg": x}, labels.clone())      # the reference rewrites the labels under fg_bg
        (grad,) = torch.autograd.grad(a * ce + b * dice, x)
        store["a.%s.logits" % tag] = logits.numpy()
        store["a.%s.labels" % tag] = labels.numpy().astype(np.uint8)
        store["a.%s.segce" % tag] = np.float64(ce.item())
        store["a.%s.segdice" % tag] = np.float64(dice.item())
        store["a.%s.grad" % tag] = grad.float().numpy()
        print("g12(a) %s: segce %.6f segdice %.6f" % (tag, float(ce), float(dice)))


def whole_model(store):
    _reference_model_imports()
    from tests._inputs import analytic_volume, fill_deterministic
    from tests._seg_inputs import P0_OUT, paint_labels, seg_model_config
    from transoar_amd.config import synthetic_targets
    from transoar.models.build import build_criterion
    from transoar.models.transoarnet import TransoarNet
    for tag, fg_bg in (("fgbg", True), ("multi", False)):
        cfg = seg_model_config(fg_bg)
        net = TransoarNet(cfg).eval()
        fill_deterministic(net)
        net = net.double()
        crit = build_criterion(cfg)
        x = analytic_volume((160, 160, 256), batch=1).double()
        targets = synthetic_targets(1, 20, seed=1)
        labels = paint_labels(targets, (160, 160, 256))
        out = net(x)
        losses = crit(out, targets, labels.clone(), net._anchors)
        coefs = cfg["loss_coefs"]
        total = sum(v * coefs[k.split("_")[0]] for k, v in losses.items())
        params = dict(net.named_parameters())
        names = ["_seg_head.weight", "_seg_head.bias", P0_OUT + ".weight", P0_OUT + ".bias"]
        grads = torch.autograd.grad(total, [params[n] for n in names])
        store["b.%s.loss_names" % tag] = np.array(list(losses.keys()))
        store["b.%s.loss_values" % tag] = np.array([float(v) for v in losses.values()])
        store["b.%s.total" % tag] = np.float64(float(total))
        store["b.%s.grad_names" % tag] = np.array(names)
        for n, g in zip(names, grads):
            store["b.%s.grad.%s" % (tag, n)] = g.numpy()
        seg = out["pred_seg"].detach()
        idx = (torch.arange(64, dtype=torch.long) * 2654435761 + 977) % seg.numel()
        store["b.%s.pred_seg_idx" % tag] = idx.numpy()
        store["b.%s.pred_seg_samples" % tag] = seg.reshape(-1)[idx].numpy()
        store["b.%s.pred_seg_abs_sum" % tag] = np.float64(float(seg.double().abs().sum()))
        print("g12(b) %s: segce %.6f segdice %.6f total %.6f" % (tag, float(losses["segce"]), float(losses["segdice"]), float(total)))


if __name__ == "__main__":
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    store = {}
    loss_level(store)
    whole_model(store)
    path = os.path.join(HERE, "g12_seg_proxy.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path))
