"""Detection validation (include/transoar_deteval.h, csrc/det_eval.hip): the other half of the reference's Trainer --
_validate() of transoar/trainer.py:112-201, which decodes one box per organ (transoar/inference.py), feeds a DetectionEvaluator
(transoar/evaluator.py, transoar/metric.py) and keeps the checkpoint whose mAP_coco is best.

The reference does that on the host: six .item() calls and three .cpu() copies per batch, then a Python triple loop over
thresholds x detections x ground truths.  Here a batch costs ONE tiny launch: there is exactly one detection per organ class
and at most one ground-truth box per class, so everything the evaluator's matching needs is (score, IoU, has_gt) per
(image, class).  `DetectionRecords.append` writes those records to device buffers with no host synchronisation; the precision /
recall arithmetic (`detection_metrics`) runs once per validation pass on the host, after one read-back.

`decode_records_torch` is the same rule as batched torch operations on the inputs' device.  It is the path for CPU tensors,
inputs the kernel does not take and TRANSOAR_DET_EVAL_HIP=0, and what the GPU tests compare the kernel with.

Two deliberate differences from the reference.  inference() returns from inside its batch loop, so the reference evaluates
sample 0 of every batch only; every sample is evaluated here.  And the validation losses are the mean over the batches of the
criterion's values, as in the reference, but stay on the device until compute().
"""
import os

import numpy as np
import torch

from . import _native
from .matcher import DenseTargets
from .train_step import TrainStep

lib = _native.bind("deteval", abi=1)
ENABLED = os.environ.get("TRANSOAR_DET_EVAL_HIP", "1") != "0"
MAX_K, MAX_QPO, MAX_N, MAX_LOSSES = 64, 4096, 1024, 32
_DT = {torch.float32: _native.F32, torch.bfloat16: _native.BF16, torch.float16: _native.F16}
RECORD_FIELDS = ("score", "iou", "has_gt", "query", "box")


# ---- the decode rule -------------------------------------------------------------------------------------------------------
def _check_inputs(logits, boxes, gt_boxes, gt_present, k):
    n, q = logits.shape[0], logits.shape[1]
    if logits.dim() != 3 or logits.shape[2] != 1 or n < 1 or k < 1 or q < k or q % k:
        raise ValueError("logits: (n, k * qpo, 1) with k = %d, got %s" % (k, tuple(logits.shape)))
    if tuple(boxes.shape) != (n, q, 6):
        raise ValueError("boxes: %s for logits %s, got %s" % ((n, q, 6), tuple(logits.shape), tuple(boxes.shape)))
    if tuple(gt_boxes.shape) != (n, k, 6) or tuple(gt_present.shape) != (n, k):
        raise ValueError("ground truth: boxes (n, k, 6) and present (n, k), got %s and %s"
                         % (tuple(gt_boxes.shape), tuple(gt_present.shape)))
    return n, q // k


def _iou_cxcyczwhd(a, b):
    """iou_3d_np (transoar/utils/bboxes.py:150-186) of box pairs (..., 6) in fp32, in numpy's order of operations; maxima,
    minima and the clamp are written as selects, like the kernel's."""
    a1, a2 = a[..., :3] - 0.5 * a[..., 3:], a[..., :3] + 0.5 * a[..., 3:]
    b1, b2 = b[..., :3] - 0.5 * b[..., 3:], b[..., :3] + 0.5 * b[..., 3:]
    da, db = a2 - a1, b2 - b1
    va, vb = da[..., 0] * da[..., 1] * da[..., 2], db[..., 0] * db[..., 1] * db[..., 2]
    lo, hi = torch.where(a1 > b1, a1, b1), torch.where(a2 < b2, a2, b2)
    e = hi - lo
    e = torch.where(e < 0, torch.zeros_like(e), e)
    inter = e[..., 0] * e[..., 1] * e[..., 2]
    return inter / ((va + vb) - inter)


def decode_records_torch(logits, boxes, gt_boxes, gt_present, k):
    """logits (n, k * qpo, 1), boxes (n, k * qpo, 6), gt_boxes (n, k, 6), gt_present (n, k) -> dict of (n, k) records: score fp32,
    iou fp32 (-1 without ground truth), has_gt uint8, query int32 (index within the organ) and box (n, k, 6) fp32.

    Per (image, class): p = 1 / (1 + exp(-x)) in fp32 over the organ's queries; the largest p wins, the lowest index among
    equals, a NaN never over a number (all NaN: index 0)."""
    n, qpo = _check_inputs(logits, boxes, gt_boxes, gt_present, k)
    x = logits.reshape(n, k, qpo).float()
    p = 1.0 / (1.0 + torch.exp(-x))
    key = torch.where(torch.isnan(p), torch.full_like(p, -1.0), p)
    best = key.amax(-1, keepdim=True)
    index = torch.arange(qpo, device=x.device).expand(n, k, qpo)
    query = torch.where(key == best, index, torch.full_like(index, qpo)).amin(-1)
    score = p.gather(-1, query[..., None])[..., 0]
    box = boxes.reshape(n, k, qpo, 6).gather(2, query[:, :, None, None].expand(n, k, 1, 6))[:, :, 0].float()
    has = gt_present != 0
    iou = torch.where(has, _iou_cxcyczwhd(box, gt_boxes.float()), torch.full_like(score, -1.0))
    return {"score": score, "iou": iou, "has_gt": has.to(torch.uint8), "query": query.to(torch.int32), "box": box}


# ---- the records -----------------------------------------------------------------------------------------------------------
class RecordsOverflow(RuntimeError):
    pass


class DetectionRecords:
    """Device buffers of one validation pass: state = {cursor, overflow} int32, the records of up to `capacity` images in
    structure-of-arrays form and fp64 sums of `n_losses` loss values.  append() never reads a device value on the host."""

    def __init__(self, capacity, k, n_losses=0, device="cpu"):
        if not (1 <= capacity <= 1 << 20 and 1 <= k and 0 <= n_losses <= MAX_LOSSES):
            raise ValueError("DetectionRecords: capacity 1..2^20, k >= 1, n_losses 0..%d" % MAX_LOSSES)
        self.capacity, self.k, self.n_losses, self.device = int(capacity), int(k), int(n_losses), torch.device(device)
        self.state = torch.zeros(2, dtype=torch.int32, device=self.device)
        dev = self.device = self.state.device            # "cuda" -> "cuda:0": the device the inputs will name
        self.score = torch.zeros(capacity, k, dtype=torch.float32, device=dev)
        self.iou = torch.zeros(capacity, k, dtype=torch.float32, device=dev)
        self.has_gt = torch.zeros(capacity, k, dtype=torch.uint8, device=dev)
        self.query = torch.zeros(capacity, k, dtype=torch.int32, device=dev)
        self.box = torch.zeros(capacity, k, 6, dtype=torch.float32, device=dev)
        self.loss_sums = torch.zeros(max(n_losses, 1), dtype=torch.float64, device=dev)
        self.launches = 0               # batches that went through the kernel (the others took the torch path)

    def reset(self):
        self.state.zero_()
        self.loss_sums.zero_()

    def usable(self, logits, boxes, gt_boxes, gt_present, losses=None):
        """Can the kernel take this batch?"""
        if not (ENABLED and self.device.type == "cuda" and self.k <= MAX_K):
            return False
        tensors = [logits, boxes, gt_boxes, gt_present] + ([] if losses is None else [losses])
        if not all(torch.is_tensor(t) and t.device == self.device and t.is_contiguous() for t in tensors):
            return False
        if logits.dtype not in _DT or boxes.dtype != logits.dtype or gt_boxes.dtype != torch.float32 or gt_present.element_size() != 1:
            return False
        if losses is not None and losses.dtype != torch.float32:
            return False
        n, q = logits.shape[0], logits.shape[1]
        return 1 <= n <= MAX_N and q % self.k == 0 and 1 <= q // self.k <= MAX_QPO

    def append(self, logits, boxes, gt_boxes, gt_present, losses=None):
        """Append the records of a batch (and add `losses`, n_losses values, to the sums).  A batch that does not fit sets the
        overflow flag and writes nothing else; to_host() raises then."""
        n, qpo = _check_inputs(logits, boxes, gt_boxes, gt_present, self.k)
        if losses is not None and tuple(losses.shape) != (self.n_losses,):
            raise ValueError("losses: %d values, got %s" % (self.n_losses, tuple(losses.shape)))
        if losses is not None and self.n_losses == 0:
            losses = None
        if self.usable(logits, boxes, gt_boxes, gt_present, losses):
            _native.launch(lib.transoar_deteval_accumulate, self.state, logits.data_ptr(), boxes.data_ptr(), _DT[logits.dtype],
                           gt_boxes.data_ptr(), gt_present.data_ptr(), _native.ptr(losses), self.n_losses, n, self.k, qpo,
                           self.state.data_ptr(), self.capacity, self.score.data_ptr(), self.iou.data_ptr(),
                           self.has_gt.data_ptr(), self.query.data_ptr(), self.box.data_ptr(), self.loss_sums.data_ptr())
            self.launches += 1
            return
        self._append_torch(decode_records_torch(logits, boxes, gt_boxes, gt_present, self.k), n, losses)

    def _append_torch(self, rec, n, losses):
        """The kernel's cursor rule in torch, also without a host read: where the batch does not fit, rows 0..n-1 are rewritten
        with what they hold."""
        if n > self.capacity:
            self.state[1:].fill_(1)
            return
        dev = self.device
        cursor = self.state[0].to(torch.int64)
        fits = (cursor >= 0) & (cursor <= self.capacity - n)
        rows = torch.where(fits, cursor, torch.zeros_like(cursor)) + torch.arange(n, device=dev)
        for name in RECORD_FIELDS:
            buf, new = getattr(self, name), rec[name].to(dev)
            buf.index_copy_(0, rows, torch.where(fits, new, buf.index_select(0, rows)))
        fits32 = fits.to(torch.int32)
        self.state.copy_(torch.stack((self.state[0] + fits32 * n, torch.maximum(self.state[1], 1 - fits32))))
        if losses is not None:
            add = losses.to(dev, torch.float64)
            self.loss_sums[:self.n_losses] += torch.where(fits, add, torch.zeros_like(add))

    def to_host(self):
        """One copy per array -> dict of numpy arrays trimmed to the cursor: score, iou, has_gt, query, box, loss_sums, count."""
        cursor, overflow = (int(v) for v in self.state.cpu())
        if overflow:
            raise RecordsOverflow("DetectionRecords: more than capacity = %d images were appended; the records hold the first %d"
                                  % (self.capacity, cursor))
        host = {name: getattr(self, name)[:cursor].cpu().numpy() for name in RECORD_FIELDS}
        host["loss_sums"] = self.loss_sums[:self.n_losses].cpu().numpy()
        host["count"] = cursor
        return host


# ---- the metric ------------------------------------------------------------------------------------------------------------
def iou_thresholds():
    """The reference evaluator's thresholds (transoar/metric.py:45-61): 0.10, 0.15, ..., 0.95."""
    nndet = np.linspace(0.1, 0.5, 9).round(2)
    coco = np.linspace(0.5, 0.95, 10).round(2)
    return np.union1d(np.union1d(np.array((0.1, 0.5, 0.75)).round(2), coco), nndet)


RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)


def precision_table(score, iou, has_gt, complete_only=False):
    """score, iou, has_gt (M, k) -> precision (18 thresholds, 101 recall steps, k) float64: Metric.compute_statistics of the
    reference for one detection and at most one ground truth per (image, class)."""
    score, iou = np.asarray(score, dtype=np.float32), np.asarray(iou, dtype=np.float32)
    has_gt = np.asarray(has_gt) != 0
    if score.ndim != 2 or score.shape != iou.shape or score.shape != has_gt.shape:
        raise ValueError("score, iou and has_gt: (M, k) each")
    if complete_only:                                   # scripts/test.py:97: only images with every class
        keep = has_gt.all(1)
        score, iou, has_gt = score[keep], iou[keep], has_gt[keep]
    thresholds = iou_thresholds()
    m, k = score.shape
    precision = np.zeros((len(thresholds), len(RECALL_THRESHOLDS), k))
    if m == 0:
        return precision
    limits = np.array([min(t, 1 - 1e-10) for t in thresholds]).astype(np.float32)
    for c in range(k):
        num_gt = int(has_gt[:, c].sum())
        if num_gt == 0:
            continue
        order = np.argsort(-score[:, c], kind="stable")
        match = has_gt[order, c][None, :] & ~(iou[order, c][None, :] < limits[:, None])            # (T, M)
        tp = np.cumsum(match, axis=1).astype(np.float32)
        fp = np.cumsum(~match, axis=1).astype(np.float32)
        rc = tp / np.float32(num_gt)
        pr = tp.astype(np.float64) / ((fp + tp).astype(np.float64) + np.spacing(1))
        pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
        for t in range(len(thresholds)):
            inds = np.searchsorted(rc[t], RECALL_THRESHOLDS, side="left")
            ok = inds < m
            precision[t, ok, c] = pr[t, inds[ok]]
    return precision


def _class_indices(subset):
    return [int(key) - 1 for key in (subset or {})]


def _mean(table):
    return float(np.mean(table)) if table.size else float("nan")


def detection_metrics(score, iou, has_gt, classes, classes_small=None, classes_mid=None, classes_large=None, per_class=False,
                      complete_only=False):
    """The reference's metric dict (Metric.compute_ap, coco (0.5, 0.95, 0.05), nnDet (0.1, 0.5, 0.05), AP at 0.10 / 0.50 /
    0.75) from the records of a validation pass.  classes: the k names; classes_small / _mid / _large: dicts keyed by class id
    (1-based, int or str), as config/<dataset>.yaml has them.  Ties between scores keep the records' order."""
    precision = precision_table(score, iou, has_gt, complete_only)
    thresholds = iou_thresholds()
    classes = list(classes)
    if len(classes) != precision.shape[2]:
        raise ValueError("classes: %d names for %d record columns" % (len(classes), precision.shape[2]))
    subsets = {"s": _class_indices(classes_small), "m": _class_indices(classes_mid), "l": _class_indices(classes_large)}
    out = {}
    for name, rows in (("coco", np.nonzero(thresholds >= 0.5)[0]), ("nndet", np.nonzero(thresholds <= 0.5)[0])):
        out["mAP_%s" % name] = _mean(precision[rows])
        for tag, idx in subsets.items():
            out["mAP_%s_%s" % (name, tag)] = _mean(precision[rows][:, :, idx])
        if per_class:
            for c, cls in enumerate(classes):
                out["mAP_%s_%s_" % (name, cls)] = _mean(precision[rows][:, :, c])
    for t in (0.1, 0.5, 0.75):
        row = int(np.nonzero(thresholds == np.round(t, 2))[0][0])
        out["AP_IoU_%.2f" % t] = _mean(precision[row])
        if per_class:
            for c, cls in enumerate(classes):
                out["AP_IoU_%.2f_%s_" % (t, cls)] = _mean(precision[row][:, c])
    return out


# ---- the validation pass ---------------------------------------------------------------------------------------------------
class Validator:
    """_validate() of the reference's Trainer without its host round trips: add() per batch, compute() per pass.

        val = Validator(model, criterion, config, classes=names, classes_small=..., classes_mid=..., classes_large=...)
        for data, labels in loader:
            val.add(data, seg_targets=labels)                 # or add(data, targets[, seg_targets])
        metrics = val.compute()                                # mAP_coco, ..., loss/total, loss/bbox, ...
        if val.is_best(metrics):
            save_checkpoint(path, model, optimizer, scheduler, epoch, val.metric_max_val)
        val.reset()
    """

    def __init__(self, model, criterion, config, classes=None, classes_small=None, classes_mid=None, classes_large=None,
                 capacity=4096, amp_dtype=torch.bfloat16, metric_max_val=0.0):
        self.model, self.criterion, self.config = model, criterion, config
        self.num_classes = int(config["num_classes"])
        self.classes = [str(c) for c in range(1, self.num_classes + 1)] if classes is None else list(classes)
        if len(self.classes) != self.num_classes:
            raise ValueError("classes: %d names for %d classes" % (len(self.classes), self.num_classes))
        self.subsets = (classes_small, classes_mid, classes_large)
        self.capacity, self.amp_dtype = int(capacity), amp_dtype
        self.metric_key, self.metric_max_val = "mAP_coco", metric_max_val
        self.records, self.loss_names = None, None
        self._one = None

    # the target handling and the weighted total of the training step, on this object's config and num_classes
    _dense = TrainStep._dense
    _weighted_total = TrainStep._weighted_total

    def reset(self):
        if self.records is not None:
            self.records.reset()

    def add(self, data, targets=None, seg_targets=None):
        """One validation batch: the model in eval mode (its mode is restored), under no_grad and autocast, the criterion, then
        the records.  targets as TrainStep.loss takes them; None: from the label volume seg_targets."""
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                targets = self._dense(data, targets, seg_targets)
                enabled = self.amp_dtype is not None and self.amp_dtype != torch.float32
                with torch.autocast(data.device.type, dtype=self.amp_dtype if enabled else torch.bfloat16, enabled=enabled):
                    out = self.model(data)
                    losses = self.criterion(out, targets, seg_targets, self.model._anchors)
                self.add_outputs(out, targets, losses)
        finally:
            self.model.train(was_training)
        return out, losses

    def add_outputs(self, out, targets, losses=None):
        """Records of a batch whose outputs (pred_logits (n, q, 1), pred_boxes (n, q, 6)) the caller already has; losses: the
        criterion's dict, or None.  After its first call (which allocates the buffers) this synchronises with nothing."""
        logits, boxes = out["pred_logits"], out["pred_boxes"]
        if not isinstance(targets, DenseTargets):
            targets = DenseTargets.from_list(targets, self.num_classes, logits.device)
        with torch.no_grad():
            if logits.dtype != boxes.dtype or logits.dtype not in _DT:
                logits, boxes = logits.float(), boxes.float()
            names = None if losses is None else ("total",) + tuple(losses.keys())
            if self.records is None:
                self.records = DetectionRecords(self.capacity, self.num_classes, 0 if names is None else len(names) + 1, logits.device)
                self.loss_names = names
                self._one = torch.ones(1, dtype=torch.float32, device=logits.device)
            vector = None
            if names is not None:
                if names != self.loss_names:
                    raise ValueError("Validator: the losses of this batch %s are not those of the pass %s" % (names, self.loss_names))
                total = self._weighted_total(losses)
                each = getattr(losses, "vector", None)
                if each is None:
                    each = torch.stack([v.detach().float() for v in losses.values()])
                # the last slot counts the batches, so that the means need no host counter
                vector = torch.cat((total.detach().float().reshape(1), each.detach().float().reshape(-1), self._one))
            present = targets.present.contiguous()
            present = present.view(torch.uint8) if present.dtype == torch.bool else present.to(torch.uint8)
            self.records.append(logits.detach().contiguous(), boxes.detach().contiguous(),
                                targets.boxes.detach().float().contiguous(), present, vector)

    def _host(self, process_group=None):
        if self.records is None:
            raise RuntimeError("Validator: nothing was added")
        host = self.records.to_host()
        if process_group is not None:
            import torch.distributed as dist
            parts = [None] * dist.get_world_size(process_group)
            dist.all_gather_object(parts, host, group=process_group)
            host = {name: np.concatenate([p[name] for p in parts]) for name in RECORD_FIELDS}          # rank-major
            host["loss_sums"] = np.sum([p["loss_sums"] for p in parts], axis=0)
            host["count"] = sum(p["count"] for p in parts)
        return host

    def predictions(self):
        """Per recorded image (boxes (k, 6), classes 1..k, scores (k,)) as numpy arrays, the format of the reference's inference()."""
        host = self._host()
        classes = np.arange(1, self.num_classes + 1)
        return [(host["box"][i], classes.copy(), host["score"][i]) for i in range(host["count"])]

    def compute(self, process_group=None, per_class=False, complete_only=False):
        """-> the metric dict of detection_metrics plus loss/<name>: the mean over the batches of the weighted total and of every
        loss of the criterion.  With a process group the records and the loss sums of all ranks are gathered first, rank-major
        (all images of rank 0, then rank 1, ...): equal scores keep that order, so the result is the one a single process gets
        when it is fed the images in that order."""
        host = self._host(process_group)
        small, mid, large = self.subsets
        metrics = detection_metrics(host["score"], host["iou"], host["has_gt"], self.classes, small, mid, large, per_class,
                                    complete_only)
        if self.loss_names is not None:
            sums = host["loss_sums"]
            batches = sums[-1]
            for name, value in zip(self.loss_names, sums[:-1]):
                metrics["loss/%s" % name] = float(value / batches) if batches else float("nan")
        return metrics

    def is_best(self, metrics):
        """trainer.py:172: a pass whose main metric is at least the best so far becomes the best (metric_max_val is what
        save_checkpoint stores)."""
        if metrics[self.metric_key] >= self.metric_max_val:
            self.metric_max_val = metrics[self.metric_key]
            return True
        return False
