"""CPU: detection targets from label volumes (transoar_amd/box_targets.py) -- the batched torch restatement against the
reference's segmentation2bbox (tests/golden/g13_box_targets.npz, make_golden_boxes.py), the criterion on DenseTargets.from_labels,
the host-side argument checks of include/transoar_boxtargets.h (no kernel is launched here) and the train step's targets=None."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests._box_inputs import CASES, NUM_CLASSES, PADDINGS, check_targets, dense_from_reference, golden_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_box_targets.npz"))


def check_against_reference(got, boxes, classes, key):
    """got: DenseTargets; boxes / classes: the reference's per-sample lists."""
    ref_boxes, ref_present = dense_from_reference(boxes, classes, len(boxes), got.boxes.shape[1])
    assert int(ref_present.sum()) == sum(int(torch.as_tensor(c).numel()) for c in classes)
    check_targets(got, ref_boxes, ref_present, key)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("tag", sorted(CASES))
def test_torch_restatement_against_g13(g13, tag, padding):
    from transoar_amd.box_targets import targets_from_labels, targets_from_labels_torch
    labels, boxes, classes = golden_case(g13, tag, padding)
    got = targets_from_labels_torch(labels, NUM_CLASSES, padding)
    check_against_reference(got, boxes, classes, "g13.torch")
    # CPU tensors take the same path through the public entry, in both label ranks and every dtype
    for dtype in (torch.uint8, torch.int16, torch.int32, torch.int64):
        for lab in (labels.to(dtype), labels[:, None].to(dtype)):
            again = targets_from_labels(lab, NUM_CLASSES, padding)
            assert torch.equal(again.boxes, got.boxes) and torch.equal(again.present, got.present)


def test_labels_outside_the_classes_are_ignored(g13):
    from transoar_amd.box_targets import targets_from_labels_torch
    labels, boxes, classes = golden_case(g13, "A", 1)
    noisy = labels.to(torch.int16).clone()
    noisy[0, 5, 0, 60:70] = NUM_CLASSES + 1
    noisy[1, 12, 16, 0:9] = -1
    check_against_reference(targets_from_labels_torch(noisy, NUM_CLASSES, 1), boxes, classes, "g13.torch")
    with pytest.raises(ValueError, match="labels"):
        targets_from_labels_torch(labels.float(), NUM_CLASSES)
    with pytest.raises(ValueError, match="labels"):
        targets_from_labels_torch(labels[0], NUM_CLASSES)


def test_criterion_on_from_labels_equals_the_reference_lists(g13):
    """The set criterion on DenseTargets.from_labels(labels) against the reference's list of dicts for the same labels: exact."""
    from transoar_amd.criterion import TransoarCriterion
    from transoar_amd.matcher import DenseTargets, Matcher
    labels, boxes, classes = golden_case(g13, "A", 1)
    n, organs, qpo = labels.shape[0], NUM_CLASSES, 27          # the flagship's 540 anchors: 27 per organ
    g = torch.Generator().manual_seed(13)
    q = organs * qpo
    anchors = torch.cat((torch.rand(q, 3, generator=g) * 0.8 + 0.1, torch.rand(q, 3, generator=g) * 0.3 + 0.05), -1)

    def outputs():
        gg = torch.Generator().manual_seed(14)
        def one():
            return {"pred_logits": torch.randn(n, q, 1, generator=gg) * 2,
                    "pred_boxes": torch.cat((torch.rand(n, q, 3, generator=gg) * 0.8 + 0.1, torch.rand(n, q, 3, generator=gg) * 0.3 + 0.02), -1)}
        out = one()
        out["aux_outputs"] = [one(), one()]
        return out
    crit = TransoarCriterion(organs, Matcher(1, 0, 0, anchor_matching=True, num_organs=organs), seg_proxy=False, seg_fg_bg=True)
    dense = DenseTargets.from_labels(labels[:, None], organs)
    assert isinstance(dense, DenseTargets) and float(dense.num_boxes) == 5
    got = crit(outputs(), dense, None, anchors)
    ref = crit(outputs(), [{"boxes": b, "labels": c} for b, c in zip(boxes, classes)], None, anchors)
    assert list(got) == list(ref)
    for k in ref:
        assert torch.equal(got[k], ref[k]), (k, float(got[k]), float(ref[k]))
    assert float(ref["bbox"]) > 0 and float(ref["cls"]) > 0


def test_boxtargets_argument_errors():
    from transoar_amd.box_targets import lib          # bound from include/transoar_boxtargets.h
    f, wb = lib.transoar_box_targets_forward, lib.transoar_box_targets_workspace_bytes
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    U8, I64 = 16, 19
    big = 1 << 30
    assert lib.transoar_boxtargets_abi_version() == 1
    # NULL required pointers
    assert f(None, U8, 2, 4, 4, 4, 20, 1, 5, p, p, p, p, big, None) == -1
    assert f(p, U8, 2, 4, 4, 4, 20, 1, 5, None, p, p, p, big, None) == -1
    assert f(p, U8, 2, 4, 4, 4, 20, 1, 5, p, None, p, p, big, None) == -1
    assert f(p, U8, 2, 4, 4, 4, 20, 1, 5, p, p, None, p, big, None) == -1
    assert f(p, U8, 2, 4, 4, 4, 20, 1, 5, p, p, p, None, big, None) == -1
    # bad dimensions
    assert f(p, U8, 0, 4, 4, 4, 20, 1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 0, 4, 4, 20, 1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 4, -1, 4, 20, 1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 4, 4, 0, 20, 1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 4, 4, 4, 0, 1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 4, 4, 4, 65, 1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 4, 4, 4, 20, -1, 5, p, p, p, p, big, None) == -2
    assert f(p, U8, 2, 4, 4, 4, 20, 1, -1, p, p, p, p, big, None) == -2
    # unknown label dtype; workspace too small
    assert f(p, 15, 2, 4, 4, 4, 20, 1, 5, p, p, p, p, big, None) == -3
    assert f(p, 20, 2, 4, 4, 4, 20, 1, 5, p, p, p, p, big, None) == -3
    need = wb(2, 64, 20)
    assert need >= 2 * 20 * 6 * 4
    assert f(p, I64, 2, 4, 4, 4, 20, 1, 5, p, p, p, p, need - 1, None) == -3
    assert f(p, I64, 2, 4, 4, 4, 20, 1, 5, p, p, p, p, 0, None) == -3
    # labels not aligned to their type
    assert f(p + 4, I64, 2, 4, 4, 4, 20, 1, 5, p, p, p, p, big, None) == -4
    # workspace: grows with the volume up to a cap, 0 for shapes the forward refuses
    assert wb(2, 160 * 160 * 256, 20) >= wb(2, 64, 20) and wb(2, 160 * 160 * 256, 20) <= 1 << 20
    assert wb(0, 64, 20) == 0 and wb(2, 0, 20) == 0 and wb(2, 64, 65) == 0


def test_local_counts_take_tensors_and_ints_alike():
    from transoar_amd.matcher import DenseTargets
    from transoar_amd.train_step import TrainStep
    present = torch.zeros(2, 20, dtype=torch.bool)
    present[0, :7] = True
    boxes = torch.zeros(2, 20, 6)
    a = TrainStep._local_counts(DenseTargets(boxes, present, 7))
    b = TrainStep._local_counts(DenseTargets(boxes, present, torch.tensor(7.0), torch.tensor(7.0)))
    c = TrainStep._local_counts(DenseTargets(boxes, present, torch.tensor(7)))
    assert a.dtype == torch.float32 and a.shape == (2,)
    assert torch.equal(a, b) and torch.equal(a, c) and a.tolist() == [7.0, 7.0]


def test_config_carries_the_reference_padding():
    from transoar_amd.config import amos_config, visceral_config
    assert visceral_config()["bbox_padding"] == 1 and amos_config()["bbox_padding"] == 1


def test_step_without_targets_needs_the_labels():
    from tests._inputs import small_model_config
    from transoar_amd.train_step import TrainStep
    from transoar_amd.transoarnet import TransoarNet, build_criterion
    cfg = small_model_config(False)
    net = TransoarNet(cfg)
    step = TrainStep(net, build_criterion(cfg), cfg, amp_dtype=None)
    with pytest.raises(ValueError, match="seg_targets"):
        step(torch.zeros(1, 1, 8, 8, 8), None)
    with pytest.raises(ValueError, match="seg_targets"):
        step.loss(torch.zeros(1, 1, 8, 8, 8), None)
    graph_step = TrainStep(net, build_criterion(cfg), cfg, amp_dtype=None, graph=True)
    with pytest.raises(ValueError, match="seg_targets"):
        graph_step.capture(torch.zeros(1, 1, 8, 8, 8), None)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference")
def test_fixture_regenerates_identically(g13):
    spec = importlib.util.spec_from_file_location("_make_golden_boxes", os.path.join(ROOT, "tests", "golden", "make_golden_boxes.py"))
    mod = importlib.util.module_from_spec(spec)
    path, modules, no_cache = list(sys.path), set(sys.modules), sys.dont_write_bytecode
    sys.dont_write_bytecode = True           # no __pycache__ next to the fixtures
    try:
        spec.loader.exec_module(mod)
        store = mod.arrays()
    finally:
        sys.dont_write_bytecode = no_cache
        sys.path[:] = path
        for name in set(sys.modules) - modules:
            if name == "transoar" or name.startswith("transoar."):
                del sys.modules[name]
    assert sorted(store) == sorted(g13.files)
    for name, arr in store.items():
        assert arr.dtype == g13[name].dtype and arr.shape == g13[name].shape and np.array_equal(arr, g13[name]), name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g13_box_targets.npz")) < 100 * 1024
