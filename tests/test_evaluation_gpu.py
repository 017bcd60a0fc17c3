"""Detection records on their kernel (csrc/det_eval.hip, include/transoar_deteval.h, transoar_amd/evaluation.py) against the
reference's inference() + DetectionEvaluator (tests/golden/g14_detection_eval.npz, make_golden_eval.py) and against the batched
torch restatement, the cursor / overflow rule, the loss sums, the launch without host synchronisation and under a captured
graph, and the Validator on the reduced-width model.

Bounds as tests/test_evaluation.py: query and has_gt exact, IoU bit-identical, score within 2^-22 absolute, metrics within 1e-12.
The torch restatement runs on CPU copies of the (rounded) inputs: IEEE fp32 there, whatever the device's torch kernels do."""
import os

import numpy as np
import pytest
import torch

from tests._eval_inputs import (CASES, CLASSES, K, LARGE, METRIC_TOL, MID, SMALL, check_records, golden_metrics, golden_records,
                                random_inputs, subset, top_two_gap)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 20, 27), (5, 20, 7), (3, 64, 54), (2, 3, 64), (1, 2, 130)]
FIELDS = ("score", "iou", "has_gt", "query", "box")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g14():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return np.load(os.path.join(root, "tests", "golden", "g14_detection_eval.npz"))


def _records(capacity, k, n_losses=0):
    from transoar_amd.evaluation import DetectionRecords
    return DetectionRecords(capacity, k, n_losses, "cuda")


def _append(buf, logits, boxes, gt, present, losses=None):
    """The kernel, on device copies (no quiet torch path in a kernel test)."""
    args = [logits.cuda(), boxes.cuda(), gt.cuda(), present.cuda().view(torch.uint8)]
    if losses is not None:
        args.append(losses.cuda())
    assert buf.usable(*args), "the kernel must take this input"
    buf.append(*args)


def _torch_records(logits, boxes, gt, present, k):
    from transoar_amd.evaluation import decode_records_torch
    return decode_records_torch(logits.cpu(), boxes.cpu(), gt.cpu(), present.cpu(), k)


def _golden_inputs(g14, tag):
    return tuple(torch.from_numpy(g14["%s.%s" % (tag, name)]) for name in ("logits", "boxes", "gt_boxes", "gt_present"))


# ---- 1. the kernel against the reference (g14) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_kernel_against_g14(g14, tag):
    from transoar_amd.evaluation import detection_metrics
    logits, boxes, gt, present = _golden_inputs(g14, tag)
    m = logits.shape[0]
    buf = _records(m, K)
    for lo, hi in ((0, 3), (3, 4), (4, m)):
        _append(buf, logits[lo:hi], boxes[lo:hi], gt[lo:hi], present[lo:hi])
    host = buf.to_host()
    assert host["count"] == m
    check_records(host, golden_records(g14, tag), "g14.kernel")
    got = detection_metrics(host["score"], host["iou"], host["has_gt"], CLASSES, subset(SMALL), subset(MID), subset(LARGE))
    want = golden_metrics(g14, tag, "sparse")
    assert sorted(got) == sorted(want)
    for name, ref in want.items():
        assert abs(got[name] - ref) <= METRIC_TOL, (tag, name, got[name], ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_kernel_against_torch_on_rounded_g14(g14, dtype):
    for tag in CASES:
        logits, boxes, gt, present = _golden_inputs(g14, tag)
        logits, boxes = logits.to(dtype), boxes.to(dtype)
        buf = _records(logits.shape[0], K)
        _append(buf, logits, boxes, gt, present)
        check_records(buf.to_host(), _torch_records(logits, boxes, gt, present, K), "g14.kernel.%s" % str(dtype)[6:])


# ---- 2. the kernel against the torch restatement on random inputs ------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_torch_on_random_inputs(shape):
    n, k, qpo = shape
    for dtype, ties in ((torch.float32, False), (torch.float32, True), (torch.bfloat16, False), (torch.float16, True)):
        logits, boxes, gt, present = random_inputs(n, k, qpo, seed=100 * k + qpo + n, dtype=dtype, ties=ties)
        # the probabilities are compared, and two evaluations may differ in the last place: distinct logits must not come closer
        assert top_two_gap(logits, k) >= 1e-5, "choose another seed: two probabilities of an organ nearly tie"
        buf = _records(n + 1, k)
        _append(buf, logits, boxes, gt, present)
        host = buf.to_host()
        assert host["count"] == n
        check_records(host, _torch_records(logits, boxes, gt, present, k), "random.kernel")
        assert buf.box[n:].abs().sum().item() == 0 and buf.score[n:].abs().sum().item() == 0          # nothing past the cursor


def test_torch_path_on_the_device_follows_the_kernel(monkeypatch):
    """TRANSOAR_DET_EVAL_HIP=0: the same buffers through the batched torch path, on the device's own torch kernels (so the IoU is
    only held to one unit in the last place of a value below 1)."""
    from transoar_amd import evaluation
    logits, boxes, gt, present = random_inputs(5, 20, 27, seed=3)
    kernel, mirror = _records(7, 20, 2), _records(7, 20, 2)
    losses = torch.tensor([0.5, 1.5])
    for lo, hi in ((0, 2), (2, 5), (0, 3)):                                     # the third batch does not fit
        _append(kernel, logits[lo:hi], boxes[lo:hi], gt[lo:hi], present[lo:hi], losses)
    monkeypatch.setattr(evaluation, "ENABLED", False)
    for lo, hi in ((0, 2), (2, 5), (0, 3)):
        args = [t[lo:hi].cuda() for t in (logits, boxes, gt, present)] + [losses.cuda()]
        assert not mirror.usable(*args)
        mirror.append(*args)
    assert kernel.state.tolist() == mirror.state.tolist() == [5, 1]
    assert torch.equal(kernel.query, mirror.query) and torch.equal(kernel.has_gt, mirror.has_gt) and torch.equal(kernel.box, mirror.box)
    assert float((kernel.score - mirror.score).abs().max()) <= 2.0 ** -22
    assert float((kernel.iou - mirror.iou).abs().max()) <= 2.0 ** -23
    assert kernel.loss_sums.tolist() == mirror.loss_sums.tolist() == [1.0, 3.0]


# ---- 3. cursor, capacity and overflow ------------------------------------------------------------------------------------------
def test_capacity_filled_exactly_then_exceeded_by_one_image():
    from transoar_amd.evaluation import RecordsOverflow
    k, qpo = 20, 27
    logits, boxes, gt, present = random_inputs(9, k, qpo, seed=11)
    want = _torch_records(logits, boxes, gt, present, k)
    losses = torch.tensor([1.0, 0.25, 3.0])
    buf = _records(8, k, 3)
    for lo, hi in ((0, 2), (2, 3), (3, 8)):                                      # 2 + 1 + 5 = capacity
        _append(buf, logits[lo:hi], boxes[lo:hi], gt[lo:hi], present[lo:hi], losses)
    assert buf.state.tolist() == [8, 0]
    host = buf.to_host()
    check_records(host, {name: v[:8] for name, v in want.items()}, "capacity.kernel")
    assert host["loss_sums"].tolist() == [3.0, 0.75, 9.0]
    kept = {name: getattr(buf, name).clone() for name in FIELDS + ("loss_sums",)}
    _append(buf, logits[8:], boxes[8:], gt[8:], present[8:], losses)              # one image too many
    assert buf.state.tolist() == [8, 1]
    for name, was in kept.items():
        assert torch.equal(getattr(buf, name), was), name
    with pytest.raises(RecordsOverflow, match="capacity"):
        buf.to_host()
    # a buffer that is one image short from the start: the batch is dropped as a whole, earlier records intact
    short = _records(7, k)
    _append(short, logits[:5], boxes[:5], gt[:5], present[:5])
    before = {name: getattr(short, name).clone() for name in FIELDS}
    _append(short, logits[5:8], boxes[5:8], gt[5:8], present[5:8])
    assert short.state.tolist() == [5, 1]
    for name, was in before.items():
        assert torch.equal(getattr(short, name), was), name
    short.reset()
    _append(short, logits[:7], boxes[:7], gt[:7], present[:7])
    check_records(short.to_host(), {name: v[:7] for name, v in want.items()}, "capacity.kernel")
    tiny = _records(1, k)
    _append(tiny, logits[:2], boxes[:2], gt[:2], present[:2])                     # a batch larger than the whole buffer
    assert tiny.state.tolist() == [0, 1] and tiny.score.abs().sum().item() == 0


def test_loss_sums_against_a_float64_host_sum():
    k, qpo, rounds = 3, 5, 40
    logits, boxes, gt, present = random_inputs(1, k, qpo, seed=5)
    g = torch.Generator().manual_seed(6)
    losses = (torch.randn(rounds, 32, generator=g) * 10 ** torch.randint(-3, 4, (rounds, 32), generator=g).float())
    buf = _records(rounds, k, 32)
    for r in range(rounds):
        _append(buf, logits, boxes, gt, present, losses[r])
    want = np.zeros(32)
    for r in range(rounds):
        want = want + losses[r].numpy().astype(np.float64)                       # the kernel's order: one fp64 add per launch
    host = buf.to_host()
    assert host["count"] == rounds and np.array_equal(host["loss_sums"], want)
    # without losses nothing is added
    _records(2, k, 4).append(logits.cuda(), boxes.cuda(), gt.cuda(), present.cuda())


# ---- 4. no host synchronisation; the launch alone in a graph -------------------------------------------------------------------
def _outputs(n, seed, dtype=torch.bfloat16):
    from transoar_amd.matcher import DenseTargets
    logits, boxes, gt, present = random_inputs(n, K, 27, seed=seed, dtype=dtype)
    out = {"pred_logits": logits.cuda(), "pred_boxes": boxes.cuda()}
    losses = {"bbox": torch.tensor(0.5 + seed, device="cuda"), "giou": torch.tensor(0.25, device="cuda"),
              "cls": torch.tensor(1.0, device="cuda")}
    return out, DenseTargets(gt.cuda(), present.cuda(), present.sum().cuda().float()), losses, (logits, boxes, gt, present)


class _NoModel(torch.nn.Module):
    _anchors = None


def test_add_outputs_synchronises_with_nothing():
    from transoar_amd.evaluation import Validator
    cfg = {"num_classes": K, "loss_coefs": {"bbox": 5, "giou": 2, "cls": 2}}
    val = Validator(_NoModel(), None, cfg, classes=CLASSES, capacity=8)
    out, targets, losses, _ = _outputs(2, 1)
    val.add_outputs(out, targets, losses)              # the first call allocates the buffers and the coefficient vector
    val.reset()
    batches = [_outputs(2, seed) for seed in (2, 3, 4)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for out, targets, losses, _ in batches:
            val.add_outputs(out, targets, losses)
        val.reset()
        for out, targets, losses, _ in batches:
            val.add_outputs(out, targets, losses)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host = val.records.to_host()
    assert host["count"] == 6 and val.records.launches == 7, "every batch went through the kernel"
    for i, (_, _, _, cpu) in enumerate(batches):
        check_records({name: host[name][2 * i:2 * i + 2] for name in FIELDS}, _torch_records(*cpu, K), "add_outputs.kernel")
    metrics = val.compute()
    assert metrics["loss/bbox"] == 3.5 and metrics["loss/cls"] == 1.0 and metrics["loss/total"] == 5 * 3.5 + 2 * 0.25 + 2 * 1.0


def test_launch_replays_in_a_graph():
    k, qpo, n = 20, 27, 2
    feeds = [random_inputs(n, k, qpo, seed=s) for s in (21, 22, 23)]
    static = [t.cuda().clone() for t in feeds[0][:3]] + [feeds[0][3].cuda().view(torch.uint8).clone()]
    static_losses = torch.zeros(2, device="cuda")
    buf = _records(3 * n + 1, k, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf.append(*static, static_losses)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    buf.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert buf.usable(*static, static_losses)
        buf.append(*static, static_losses)
    assert buf.state.tolist() == [0, 0], "capturing launches nothing"
    eager = _records(3 * n + 1, k, 2)
    for i, (logits, boxes, gt, present) in enumerate(feeds):
        losses = torch.tensor([1.0 + i, 0.5])
        for dst, src in zip(static, (logits, boxes, gt, present.view(torch.uint8))):
            dst.copy_(src)
        static_losses.copy_(losses)
        graph.replay()
        torch.cuda.synchronize()
        _append(eager, logits, boxes, gt, present, losses)
        assert buf.state.tolist() == eager.state.tolist() == [n * (i + 1), 0]
    for name in FIELDS + ("loss_sums",):
        assert torch.equal(getattr(buf, name), getattr(eager, name)), name
    assert buf.loss_sums.tolist() == [6.0, 1.5]
    assert not torch.equal(buf.query[:n], buf.query[n:2 * n])


# ---- 5. the Validator on the reduced-width model --------------------------------------------------------------------------------
def test_validator_on_the_reduced_model():
    from tests._inputs import small_model_config
    from tests._seg_inputs import paint_labels
    from transoar_amd.box_targets import targets_from_labels
    from transoar_amd.config import synthetic_targets
    from transoar_amd.evaluation import Validator, detection_metrics
    from transoar_amd.transoarnet import TransoarNet, build_criterion
    cfg = small_model_config(False, use_cuda=True)
    torch.manual_seed(0)
    net = TransoarNet(cfg)
    with torch.no_grad():                       # the heads start at zero in the reference: every query alike
        for prm in net.parameters():
            if prm.dim() > 1 and float(prm.abs().max()) == 0:
                torch.nn.init.xavier_uniform_(prm)
    net = net.cuda().train()
    val = Validator(net, build_criterion(cfg), cfg, classes=CLASSES, classes_small=subset(SMALL), classes_mid=subset(MID),
                    classes_large=subset(LARGE), capacity=4)
    g = torch.Generator(device="cuda").manual_seed(5)
    wants, totals = [], []
    for seed in (1, 2):
        x = torch.rand(1, 1, 160, 160, 256, device="cuda", generator=g)
        labels = paint_labels(synthetic_targets(1, 20, seed=seed), (160, 160, 256)).to(torch.uint8).cuda()
        out, losses = val.add(x, None, labels)                              # targets=None: from the label volume
        assert net.training and not out["pred_logits"].requires_grad
        dense = targets_from_labels(labels, 20, cfg["bbox_padding"])
        assert int(dense.present.sum()) >= 15
        wants.append(_torch_records(out["pred_logits"].float(), out["pred_boxes"].float(), dense.boxes, dense.present, 20)
                     if out["pred_logits"].dtype != out["pred_boxes"].dtype else
                     _torch_records(out["pred_logits"], out["pred_boxes"], dense.boxes, dense.present, 20))
        totals.append({k: float(v) for k, v in losses.items()})
    host = val.records.to_host()
    assert host["count"] == 2 and val.records.launches == 2, "both batches went through the kernel"
    want = {name: torch.cat([w[name] for w in wants]) for name in FIELDS}
    check_records(host, want, "validator.kernel")
    metrics = val.compute(per_class=True)
    ref = detection_metrics(host["score"], host["iou"], host["has_gt"], CLASSES, subset(SMALL), subset(MID), subset(LARGE), True)
    for name, value in ref.items():
        assert metrics[name] == value, name
    print("validator: mAP_coco %.4f mAP_nndet %.4f AP10 %.4f" % (metrics["mAP_coco"], metrics["mAP_nndet"], metrics["AP_IoU_0.10"]))
    for name in totals[0]:
        mean = (totals[0][name] + totals[1][name]) / 2
        assert abs(metrics["loss/" + name] - mean) <= 1e-6 * max(abs(mean), 1.0), name
    assert val.is_best(metrics) and val.metric_max_val == metrics["mAP_coco"]
