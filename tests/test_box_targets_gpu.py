"""Detection targets from label volumes on their kernels (csrc/box_targets.hip, include/transoar_boxtargets.h,
transoar_amd/box_targets.py) against the reference's segmentation2bbox (tests/golden/g13_box_targets.npz, make_golden_boxes.py)
and the batched torch restatement, and in the training step: eager and as the first nodes of the captured step (targets=None).

Bounds as tests/test_box_targets.py: present exact, boxes within 2^-22 absolute and bit-identical, absent rows zero."""
import os

import numpy as np
import pytest
import torch

from tests._box_inputs import CASES, NUM_CLASSES, PADDINGS, blob_volume, check_targets, dense_from_reference, golden_case
from tests._seg_inputs import paint_labels

pytestmark = pytest.mark.gpu

DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g13():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return np.load(os.path.join(root, "tests", "golden", "g13_box_targets.npz"))


def _kernels(labels, k, padding=1, workspace=None):
    from transoar_amd import box_targets
    assert box_targets.usable(labels, k), "the kernels must take this input (no quiet torch path in a kernel test)"
    return box_targets.targets_from_labels(labels, k, padding, workspace=workspace)


# ---- 1. kernels against the reference (g13) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [4, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d)[6:] for d in DTYPES])
def test_kernels_against_g13(g13, dtype, rank):
    for tag in sorted(CASES):
        for padding in PADDINGS:
            labels, boxes, classes = golden_case(g13, tag, padding)
            lab = labels.to(dtype).cuda()
            if rank == 5:
                lab = lab[:, None]
            kept = lab.clone()
            got = _kernels(lab, NUM_CLASSES, padding)
            assert got.boxes.is_cuda and got.num_boxes.is_cuda and got.n_present.is_cuda
            assert torch.equal(lab, kept)
            ref_boxes, ref_present = dense_from_reference(boxes, classes, len(boxes))
            check_targets(got, ref_boxes, ref_present, "g13.kernels")


# ---- 2. kernels against the torch restatement on random blob volumes --------------------------------------------------------
def _against_torch(shape, k, dtype, seed):
    from transoar_amd.box_targets import targets_from_labels_torch
    lab = blob_volume(shape, k, dtype, seed).cuda()
    ref = targets_from_labels_torch(lab, k, 1)
    got = _kernels(lab, k, 1)
    check_targets(got, ref.boxes, ref.present, "blobs.kernels")
    return int(ref.present.sum())


@pytest.mark.parametrize("k", [1, 20, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d)[6:] for d in DTYPES])
@pytest.mark.parametrize("shape", [(1, 5, 6, 7), (2, 13, 17, 70), (1, 40, 48, 64)], ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_torch_on_blobs(shape, dtype, k):
    found = _against_torch(shape, k, dtype, seed=100 * k + shape[1])
    if shape == (1, 5, 6, 7):
        assert found == 0                     # extents of at most 4 on the first axis: no box is possible


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["uint8", "int64"])
def test_kernels_against_torch_flagship(dtype):
    assert _against_torch((2, 160, 160, 256), NUM_CLASSES, dtype, seed=7) > 0


# ---- 3. reproducibility, independence of the workspace's contents -------------------------------------------------------------
def test_bitwise_reproducible_whatever_the_workspace_held(g13):
    from transoar_amd import box_targets
    labels, _, _ = golden_case(g13, "A", 1)
    lab = labels.cuda()
    n, vox = lab.shape[0], lab[0].numel()
    words = box_targets.workspace_bytes(n, vox, NUM_CLASSES) // 4
    assert words >= n * NUM_CLASSES * 6
    first = _kernels(lab, NUM_CLASSES, 1)
    assert int(first.present.sum()) == 5
    g = torch.Generator(device="cuda").manual_seed(3)
    spaces = [None,
              torch.full((words,), -1, dtype=torch.int32, device="cuda"),                            # 0xFF bytes
              torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int32, device="cuda", generator=g)]
    for ws in spaces:
        again = _kernels(lab, NUM_CLASSES, 1, workspace=ws)
        assert torch.equal(again.boxes.view(torch.int32), first.boxes.view(torch.int32))
        assert torch.equal(again.present, first.present)
        assert torch.equal(again.num_boxes, first.num_boxes) and torch.equal(again.n_present, first.n_present)


# ---- 4. the bare op under a captured graph ----------------------------------------------------------------------------------
def test_op_replays_in_a_graph(g13):
    from transoar_amd import box_targets
    labels, _, _ = golden_case(g13, "A", 1)
    lab_a = labels.cuda()
    lab_b = labels.flip(1, 2, 3).contiguous().cuda()
    n, k = lab_a.shape[0], NUM_CLASSES
    static = torch.zeros_like(lab_a)
    boxes = torch.empty(n, k, 6, device="cuda")
    present = torch.empty(n, k, dtype=torch.bool, device="cuda")
    counts = torch.empty(2, device="cuda")
    ws = torch.empty(box_targets.workspace_bytes(n, lab_a[0].numel(), k) // 4, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        box_targets.box_targets_into(static, k, 1, 5, boxes, present, counts, ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        box_targets.box_targets_into(static, k, 1, 5, boxes, present, counts, ws)
    for lab in (lab_a, lab_b, lab_a):
        static.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        eager = _kernels(lab, k, 1)
        assert torch.equal(boxes.view(torch.int32), eager.boxes.view(torch.int32))
        assert torch.equal(present, eager.present)
        assert float(counts[0]) == float(eager.num_boxes) == float(counts[1]) == float(eager.n_present)
    assert not torch.equal(_kernels(lab_a, k, 1).boxes, _kernels(lab_b, k, 1).boxes)


# ---- 5. the training step with targets=None ---------------------------------------------------------------------------------
def _flagship_model(seg_proxy, seed=0):
    from transoar_amd.config import synthetic_bbox_properties, visceral_config
    from transoar_amd.transoarnet import TransoarNet, build_criterion
    cfg = visceral_config(refine=True, use_cuda=True)
    cfg["backbone"]["use_seg_proxy_loss"] = seg_proxy
    cfg["bbox_properties"] = synthetic_bbox_properties(cfg["num_classes"], seed=0)
    torch.manual_seed(seed)
    model = TransoarNet(cfg).cuda()
    return cfg, model, build_criterion(cfg)


def _flagship_labels(cfg):
    """lab1: every class's median box of cfg["bbox_properties"] painted into both samples (targets next to the anchors);
    lab2: the boxes of synthetic_targets(seed=1)."""
    from transoar_amd.config import synthetic_targets
    k = cfg["num_classes"]
    median = {"boxes": torch.tensor([cfg["bbox_properties"][str(c)]["median"] for c in range(1, k + 1)]),
              "labels": torch.arange(1, k + 1)}
    lab1 = paint_labels([median, median], cfg["volume_shape"]).to(torch.uint8).cuda()
    lab2 = paint_labels(synthetic_targets(2, k, seed=1), cfg["volume_shape"]).to(torch.uint8).cuda()
    return lab1, lab2


@pytest.mark.parametrize("seg_proxy", [True, False], ids=["seg_proxy", "no_seg_proxy"])
def test_step_computes_its_targets_from_the_labels(seg_proxy):
    """Eager and captured steps with targets=None against the eager step on targets_from_labels(labels).

    The two label volumes must move the total by more than ten times the 2e-3 tolerance, or a replay that ignored the labels
    would pass.  Observed on an MI355X, labels painted from the per-class median boxes / from synthetic_targets(seed=1): totals
    17.1369 / 25.7094 with the seg proxy on, 13.6910 / 22.2972 with it off (eager with targets=None, eager with the targets
    given and the replays agreed to the last printed digit); the totals are printed."""
    from transoar_amd.box_targets import targets_from_labels
    from transoar_amd.train_step import TrainStep, build_optimizer
    cfg, model, crit = _flagship_model(seg_proxy)
    opt = build_optimizer(model, cfg)
    for group in opt.param_groups:         # replays must not move the weights: every replay is compared with an eager pass
        group["lr"] = 0.0
    step = TrainStep(model, crit, cfg, optimizer=opt, amp_dtype=torch.bfloat16, graph=True)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand(2, 1, *cfg["volume_shape"], device="cuda", generator=g)
    lab1, lab2 = _flagship_labels(cfg)
    k = cfg["num_classes"]

    def eager(labels, targets):
        side = step.capture_stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            total = float(step._eager_fwd_bwd(x, targets, labels)[0])
        torch.cuda.current_stream().wait_stream(side)
        return total

    t1, t2 = targets_from_labels(lab1, k, cfg["bbox_padding"]), targets_from_labels(lab2, k, cfg["bbox_padding"])
    assert int(t1.present.sum()) >= k and int(t2.present.sum()) >= k, "most classes survive the painting"
    e1, e2 = eager(lab1, None), eager(lab2, None)
    g1, g2 = eager(lab1, t1), eager(lab2, t2)
    print("eager totals: labels 1 %.6f (given targets %.6f), labels 2 %.6f (given targets %.6f)" % (e1, g1, e2, g2))
    assert abs(e1 - g1) <= 2e-3 * abs(g1), (e1, g1)
    assert abs(e2 - g2) <= 2e-3 * abs(g2), (e2, g2)
    assert abs(e1 - e2) > 2e-2 * abs(e1), "the two label volumes must separate the totals: %r %r" % (e1, e2)
    step.capture(x, None, lab1, warmup=1)
    r1 = float(step(x, None, lab1)[0])
    r2 = float(step(x, None, lab2.clone())[0])
    r1b = float(step(x, None, lab1.clone())[0])
    print("replay totals: labels 1 %.6f, labels 2 %.6f, labels 1 again %.6f" % (r1, r2, r1b))
    assert abs(r1 - e1) <= 2e-3 * abs(e1), (r1, e1)
    assert abs(r2 - e2) <= 2e-3 * abs(e2), (r2, e2)
    assert abs(r1b - e1) <= 2e-3 * abs(e1), (r1b, e1)
    assert torch.equal(step._static_t.boxes, t1.boxes) and torch.equal(step._static_t.present, t1.present)
    with pytest.raises(RuntimeError, match="captured with targets=None"):
        step(x, t1, lab1)
    with pytest.raises(RuntimeError, match="seg_targets"):
        step(x, None)
