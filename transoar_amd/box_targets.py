"""Detection targets from label volumes (include/transoar_boxtargets.h, csrc/box_targets.hip): what the reference's collator
computes on the host for every batch -- transoar/data/dataloader.py:56, segmentation2bbox(labels, bbox_padding, 'cxcyczwhd',
normalize=True) of transoar/utils/bboxes.py:45-96 (unique(), then nonzero() / min / max per class) -- as two launches on the
device, straight into the DenseTargets the criterion takes, with no host synchronisation: the box count and the number of
present classes stay device scalars, so the call can be the first node of the captured training step.

`targets_from_labels_torch` is the same rule as batched torch operations (per axis one scatter of the labels into an occupancy
table, no loop over voxels, classes or samples).  It is the path for CPU tensors, inputs the kernels do not take and
TRANSOAR_BOX_TARGETS_HIP=0, and what the GPU tests compare the kernels with.

One difference from the reference, in both paths: labels that are 0, negative or above num_classes are ignored (the reference
would emit a class above num_classes, for which DenseTargets has no slot).
"""
import os

import torch

from . import _native
from .matcher import DenseTargets

lib = _native.bind("boxtargets", abi=1)
ENABLED = os.environ.get("TRANSOAR_BOX_TARGETS_HIP", "1") != "0"
MAX_K = 64
_LABEL_DT = {torch.uint8: 16, torch.int16: 17, torch.int32: 18, torch.int64: 19}


def _volume(labels):
    """(N, 1, D, H, W) or (N, D, H, W) -> (N, D, H, W)"""
    if not torch.is_tensor(labels) or labels.dim() not in (4, 5) or (labels.dim() == 5 and labels.shape[1] != 1):
        raise ValueError("labels: a tensor of shape (N, 1, D, H, W) or (N, D, H, W), got %s"
                         % (str(tuple(labels.shape)) if torch.is_tensor(labels) else type(labels).__name__))
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError("labels: an integer tensor, got %s" % labels.dtype)
    return labels[:, 0] if labels.dim() == 5 else labels


def usable(labels, num_classes):
    """Can the kernels take this label tensor?"""
    return (ENABLED and torch.is_tensor(labels) and labels.is_cuda and labels.dtype in _LABEL_DT and labels.dim() in (4, 5)
            and labels.numel() > 0 and 1 <= num_classes <= MAX_K and labels.shape[0] <= 65535)


def workspace_bytes(n, voxels_per_sample, num_classes):
    return int(lib.transoar_box_targets_workspace_bytes(n, voxels_per_sample, num_classes))


def box_targets_into(labels, num_classes, padding, min_extent, boxes, present, counts, workspace=None):
    """The kernel pair on the current stream, writing boxes (N, k, 6) fp32, present (N, k) uint8 / bool and counts (2) fp32 in
    place.  workspace: a device tensor of at least workspace_bytes(...) bytes (any contents), else one is allocated."""
    vol = _volume(labels).contiguous()
    n, sx, sy, sz = vol.shape
    k = int(num_classes)
    assert boxes.shape == (n, k, 6) and boxes.dtype == torch.float32 and boxes.is_contiguous()
    assert present.shape == (n, k) and present.element_size() == 1 and present.is_contiguous()
    assert counts.numel() == 2 and counts.dtype == torch.float32 and counts.is_contiguous()
    need = workspace_bytes(n, sx * sy * sz, k)
    if workspace is None:
        workspace = torch.empty(max(need, 4) // 4, dtype=torch.int32, device=vol.device)
    _native.launch(lib.transoar_box_targets_forward, vol, vol.data_ptr(), _LABEL_DT[vol.dtype], n, sx, sy, sz, k, int(padding),
                   int(min_extent), boxes.data_ptr(), present.data_ptr(), counts.data_ptr(), workspace.data_ptr(),
                   workspace.numel() * workspace.element_size())


def targets_from_labels(labels, num_classes, padding=1, min_extent=5, workspace=None):
    """labels (N, 1, D, H, W) or (N, D, H, W), uint8 / int16 / int32 / int64 -> DenseTargets(boxes (N, k, 6), present (N, k)
    bool, num_boxes, n_present); the two counts are DEVICE scalars (nothing is read back)."""
    if not usable(labels, num_classes):
        return targets_from_labels_torch(labels, num_classes, padding, min_extent)
    vol = _volume(labels)
    n, k = vol.shape[0], int(num_classes)
    boxes = torch.empty(n, k, 6, dtype=torch.float32, device=vol.device)
    present = torch.empty(n, k, dtype=torch.bool, device=vol.device)
    counts = torch.empty(2, dtype=torch.float32, device=vol.device)
    box_targets_into(vol, k, padding, min_extent, boxes, present, counts, workspace)
    return DenseTargets(boxes, present, counts[0], counts[1])


def _extent(vol, axis, k):
    """Smallest and largest index along `axis` (1..3) of every class: two (N, k) int64 tensors, (size, -1) where absent."""
    n, size = vol.shape[0], vol.shape[axis]
    idx = vol.movedim(axis, 1).reshape(n, size, -1)
    occupied = torch.zeros(n, size, k + 1, dtype=torch.bool, device=vol.device)
    occupied.scatter_(2, idx, True)                   # duplicates all write True
    occupied = occupied[:, :, 1:]
    pos = torch.arange(size, device=vol.device)[None, :, None]
    lo = torch.where(occupied, pos, size).amin(1)
    hi = torch.where(occupied, pos, -1).amax(1)
    return lo, hi


def targets_from_labels_torch(labels, num_classes, padding=1, min_extent=5):
    """The rule of transoar/utils/bboxes.py:45-96 in batched torch, on the labels' device; fp32 in the reference's order of
    operations.  num_boxes and n_present are 0-d tensors here too."""
    vol = _volume(labels)
    k = int(num_classes)
    vol = vol.to(torch.int64)
    vol = torch.where((vol >= 1) & (vol <= k), vol, torch.zeros_like(vol))
    los, his = zip(*(_extent(vol, a, k) for a in (1, 2, 3)))
    lo, hi = torch.stack(los, -1), torch.stack(his, -1)                # (N, k, 3)
    present = ((hi >= lo) & (hi - lo >= min_extent)).all(-1)
    size = torch.tensor(vol.shape[1:], dtype=torch.float32, device=vol.device)
    lo = (lo.float() - padding).clamp(min=0)
    hi = torch.minimum(hi.float() + padding, size)
    lo, hi = lo / size, hi / size
    boxes = torch.cat(((hi + lo) / 2, hi - lo), -1)
    boxes = torch.where(present[:, :, None], boxes, torch.zeros_like(boxes))
    count = present.sum().float()
    return DenseTargets(boxes, present, count, count.clone())
