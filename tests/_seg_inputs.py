"""Inputs of the segmentation proxy tests, shared with tests/golden/make_golden_seg.py."""
import torch

# g12(a): (tag, K, fg_bg, shape (N, D, H, W), label range, absent class or None, seed)
LOSS_CASES = (
    ("k2_fgbg", 2, True, (2, 7, 9, 11), 21, None, 0),       # multi-class labels in, mapped to (label > 0)
    ("k2_all_bg", 2, True, (1, 4, 5, 6), 1, 1, 1),          # the foreground class absent from the whole batch
    ("k21", 21, False, (2, 3, 5, 7), 21, 5, 2),             # class 5 absent from the whole batch
)
LOSS_GRAD_COEFS = (0.7, 1.3)          # the stored gradient is that of a * segce + b * segdice


def loss_case_inputs(k, shape, label_range, absent, seed):
    """-> (logits fp32 (N, K, D, H, W), labels int64 (N, 1, D, H, W))"""
    g = torch.Generator().manual_seed(seed)
    n = shape[0]
    logits = 2.0 * torch.randn((n, k) + tuple(shape[1:]), generator=g)
    labels = torch.randint(0, label_range, (n, 1) + tuple(shape[1:]), generator=g)
    if absent is not None:
        labels[labels == absent] = 0
    return logits, labels


def paint_labels(targets, spatial):
    """Label volume (N, 1, D, H, W) int64 consistent with the boxes of `targets` (list of {"boxes": (O, 6) cx cy cz w h d in
    [0, 1], "labels": (O,)}): every class's box interior painted with its id, in the order of the list (later over earlier);
    box axes x, y, z along D, H, W."""
    vol = torch.zeros((len(targets), 1) + tuple(spatial), dtype=torch.int64)
    for i, t in enumerate(targets):
        for box, lab in zip(t["boxes"].cpu().double(), t["labels"].cpu()):
            lo = [int(round(float(box[a] - box[a + 3] / 2) * spatial[a])) for a in range(3)]
            hi = [int(round(float(box[a] + box[a + 3] / 2) * spatial[a])) for a in range(3)]
            lo = [max(0, v) for v in lo]
            hi = [min(spatial[a], hi[a]) for a in range(3)]
            vol[i, 0, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = int(lab)
    return vol


def seg_model_config(fg_bg, use_cuda=False):
    """tests/_inputs.py::small_model_config with the segmentation proxy on."""
    from tests._inputs import small_model_config
    cfg = small_model_config(False, use_cuda)
    cfg["backbone"].update(use_seg_proxy_loss=True, fg_bg=fg_bg)
    return cfg


P0_OUT = "_backbone._decoder._out.0"           # the P0 output convolution (3x3x3, start_channels out)
