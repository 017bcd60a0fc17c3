"""CPU: the segmentation proxy loss of the torch mirror (TransoarCriterion.loss_segmentation, SoftDiceLoss, the 1x1x1 head) against
the reference's values in tests/golden/g12_seg_proxy.npz (make_golden_seg.py), and the host-side argument checks of every entry of
include/transoar_segproxy.h (no kernel is launched here)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.torch_ref import msda3d_core_torch
from tests._inputs import analytic_volume, fill_deterministic
from tests._seg_inputs import LOSS_CASES, LOSS_GRAD_COEFS, P0_OUT, paint_labels, seg_model_config

def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_seg_proxy.npz"))


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_mirror_loss_level_against_g12a(g12, case):
    from transoar_amd.criterion import TransoarCriterion
    tag, k, fg_bg = case[:3]
    logits = torch.from_numpy(g12["a.%s.logits" % tag]).double().requires_grad_()
    labels = torch.from_numpy(g12["a.%s.labels" % tag]).long()
    kept = labels.clone()
    crit = TransoarCriterion(20, None, seg_proxy=True, seg_fg_bg=fg_bg)
    ce, dice = crit.loss_segmentation({"pred_seg": logits}, labels)
    assert torch.equal(labels, kept), "the caller's labels must not be modified"
    assert abs(ce.item() - float(g12["a.%s.segce" % tag])) <= 1e-10 * abs(float(g12["a.%s.segce" % tag]))
    assert abs(dice.item() - float(g12["a.%s.segdice" % tag])) <= 1e-10 * abs(float(g12["a.%s.segdice" % tag]))
    a, b = LOSS_GRAD_COEFS
    (grad,) = torch.autograd.grad(a * ce + b * dice, logits)
    assert relerr(grad, g12["a.%s.grad" % tag]) <= 1e-6          # the stored gradient is rounded to fp32


@pytest.fixture
def debug_core():
    from transoar_amd import ms_deform_attn as mod
    prev = mod.register_debug_core(msda3d_core_torch)
    yield
    mod.register_debug_core(prev)


@pytest.mark.parametrize("tag,fg_bg", [("fgbg", True), ("multi", False)])
def test_mirror_whole_model_against_g12b(g12, debug_core, tag, fg_bg):
    from transoar_amd.config import synthetic_targets
    from transoar_amd.transoarnet import TransoarNet, build_criterion
    cfg = seg_model_config(fg_bg)
    net = TransoarNet(cfg).eval()
    fill_deterministic(net)
    net = net.double()                   # g12(b) is an fp64 fixture (make_golden_seg.py: the head's bias gradient cancels)
    targets = synthetic_targets(1, 20, seed=1)
    labels = paint_labels(targets, (160, 160, 256))
    out = net(analytic_volume((160, 160, 256), batch=1).double())
    seg = out["pred_seg"].detach().contiguous().reshape(-1)
    assert relerr(seg[torch.from_numpy(g12["b.%s.pred_seg_idx" % tag])], g12["b.%s.pred_seg_samples" % tag]) <= 1e-9
    losses = build_criterion(cfg)(out, targets, labels, net._anchors)
    assert list(losses.keys()) == list(g12["b.%s.loss_names" % tag])
    for (k, v), ref in zip(losses.items(), g12["b.%s.loss_values" % tag]):
        tol = 1e-9 if k.startswith("seg") else 1e-6         # the mirror's box terms are fp32 (criterion.py: .float())
        assert abs(v.item() - ref) <= tol * max(abs(ref), 1e-3), (k, v.item(), ref)
    coefs = cfg["loss_coefs"]
    total = sum(v * coefs[k.split("_")[0]] for k, v in losses.items())
    params = dict(net.named_parameters())
    names = list(g12["b.%s.grad_names" % tag])
    assert names[:2] == ["_seg_head.weight", "_seg_head.bias"] and names[2].startswith(P0_OUT)
    grads = torch.autograd.grad(total, [params[n] for n in names])
    for n, g in zip(names, grads):
        assert relerr(g, g12["b.%s.grad.%s" % (tag, n)]) <= 1e-7, n


def test_segproxy_argument_errors():
    from transoar_amd.seg_proxy import lib          # bound from include/transoar_segproxy.h
    hf, hb = lib.transoar_seg_head_forward, lib.transoar_seg_head_backward
    lf, lb = lib.transoar_seg_loss_forward, lib.transoar_seg_loss_backward
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    NCDHW, NDHWC, F32, BF16, F16, U8, I64 = 0, 1, 0, 2, 3, 16, 19
    # head forward: NULL, C / K / N out of range, dtype, layout
    assert hf(None, NDHWC, BF16, p, p, 2, 8, 24, 21, p, None) == -1
    assert hf(p, NDHWC, BF16, p, None, 2, 8, 24, 21, p, None) == -1
    assert hf(p, NDHWC, BF16, p, p, 2, 8, 65, 21, p, None) == -2
    assert hf(p, NDHWC, BF16, p, p, 2, 8, 0, 21, p, None) == -2
    assert hf(p, NDHWC, BF16, p, p, 2, 8, 24, 33, p, None) == -2
    assert hf(p, NDHWC, BF16, p, p, 0, 8, 24, 21, p, None) == -2
    assert hf(p, NDHWC, F16, p, p, 2, 8, 24, 21, p, None) == -3
    assert hf(p, 2, BF16, p, p, 2, 8, 24, 21, p, None) == -4
    # head backward: dx may be NULL (not wanted), dw / db / workspace may not
    assert hb(p, NDHWC, BF16, p, NDHWC, p, 2, 8, 24, 21, None, p, p, None, None) == -1
    assert hb(p, NDHWC, BF16, p, NDHWC, p, 2, 8, 24, 21, p, None, p, p, None) == -1
    assert hb(p, NDHWC, BF16, p, NDHWC, p, 2, 8, 64, 0, p, p, p, p, None) == -2
    assert hb(p, NDHWC, 1, p, NDHWC, p, 2, 8, 24, 21, p, p, p, p, None) == -3
    assert hb(p, NDHWC, BF16, p, 7, p, 2, 8, 24, 21, p, p, p, p, None) == -4
    # loss forward: K >= 2, label dtypes
    assert lf(p, NDHWC, BF16, None, U8, 2, 8, 21, 0, 1e-5, 1e-5, p, p, p, None) == -1
    assert lf(p, NDHWC, BF16, p, U8, 2, 8, 1, 0, 1e-5, 1e-5, p, p, p, None) == -2
    assert lf(p, NDHWC, BF16, p, U8, 2, 8, 33, 0, 1e-5, 1e-5, p, p, p, None) == -2
    assert lf(p, NDHWC, BF16, p, U8, 2, 0, 21, 0, 1e-5, 1e-5, p, p, p, None) == -2
    assert lf(p, NDHWC, F16, p, U8, 2, 8, 21, 0, 1e-5, 1e-5, p, p, p, None) == -3
    assert lf(p, NDHWC, BF16, p, 15, 2, 8, 21, 0, 1e-5, 1e-5, p, p, p, None) == -3      # no bool / int8 labels
    assert lf(p, -1, BF16, p, I64, 2, 8, 21, 0, 1e-5, 1e-5, p, p, p, None) == -4
    # loss backward: the upstream gradient pointer is required
    assert lb(p, NCDHW, F32, p, I64, 2, 8, 21, 0, p, None, p, None) == -1
    assert lb(p, NCDHW, F32, p, I64, 2, 8, 40, 0, p, p, p, None) == -2
    assert lb(p, NCDHW, F32, p, 3, 2, 8, 21, 0, p, p, p, None) == -3
    assert lb(p, 5, F32, p, I64, 2, 8, 21, 0, p, p, p, None) == -4
    # workspace: enough for the head backward's and the loss forward's slabs, 0 for impossible shapes
    assert lib.transoar_seg_workspace_bytes(24, 21) >= 4 * 1024 * (24 * 21 + 21)
    assert lib.transoar_seg_workspace_bytes(0, 21) >= 4 * 1024 * (1 + 3 * 21)
    assert lib.transoar_seg_workspace_bytes(65, 21) == 0 and lib.transoar_seg_workspace_bytes(24, 0) == 0


def test_paths_that_stay_on_torch():
    """CPU tensors and unsupported shapes keep the torch code; the kernels' usability checks say so."""
    from transoar_amd import seg_proxy
    conv = torch.nn.Conv3d(4, 2, kernel_size=1)
    x = torch.zeros(1, 4, 2, 2, 2)
    assert not seg_proxy.head_usable(x, conv)
    assert not seg_proxy.losses_usable(torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2, dtype=torch.long))


def test_capture_without_seg_targets_is_a_clear_error():
    """With the seg proxy on, TrainStep.capture needs the label volume (it becomes a static input of the graph)."""
    from transoar_amd.config import synthetic_targets
    from transoar_amd.train_step import TrainStep
    from transoar_amd.transoarnet import TransoarNet, build_criterion
    cfg = seg_model_config(True)
    net = TransoarNet(cfg)
    step = TrainStep(net, build_criterion(cfg), cfg, amp_dtype=None, graph=True)
    with pytest.raises(RuntimeError, match="pass the label volume as seg_targets"):
        step.capture(torch.zeros(1, 1, 8, 8, 8), synthetic_targets(1, 20, seed=1))
