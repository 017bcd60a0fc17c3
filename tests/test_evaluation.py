"""CPU: detection validation (transoar_amd/evaluation.py) -- the batched torch decode and the vectorised metric against the
reference's inference() + DetectionEvaluator (tests/golden/g14_detection_eval.npz, make_golden_eval.py), the record buffers, the
host-side argument checks of include/transoar_deteval.h (no kernel is launched here), the Validator on a reduced-width model and
a 2-rank gloo compute().

Bounds: the chosen query and has_gt exact, the IoU bit-identical (same fp32 operations in the same order), the score within
2^-22 absolute (tests/_eval_inputs.py::SCORE_TOL), every metric within 1e-12 (float64 means of the same precision table)."""
import ctypes
import importlib.util
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests._eval_inputs import (CASES, CLASSES, K, LARGE, METRIC_TOL, MID, SMALL, case_inputs, check_records, golden_metrics,
                                golden_records, random_inputs, subset)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUME = (32, 32, 64)      # as tests/test_data_parallel.py: a small volume keeps the CPU suite fast


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(os.path.join(golden_dir, "g14_detection_eval.npz"))


def _golden_inputs(g14, tag):
    return tuple(torch.from_numpy(g14["%s.%s" % (tag, name)]) for name in ("logits", "boxes", "gt_boxes", "gt_present"))


def _metrics(rec, **kw):
    from transoar_amd.evaluation import detection_metrics
    return detection_metrics(rec["score"], rec["iou"], rec["has_gt"], CLASSES, subset(SMALL), subset(MID), subset(LARGE), **kw)


def _check_metrics(got, want, key):
    assert sorted(got) == sorted(want), key
    for name, ref in want.items():
        assert abs(got[name] - ref) <= METRIC_TOL, (key, name, got[name], ref)


# ---- 1. torch path + metric against the reference (g14) ----------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_torch_path_and_metrics_against_g14(g14, tag):
    from transoar_amd.evaluation import DetectionRecords, decode_records_torch
    logits, boxes, gt, present = _golden_inputs(g14, tag)
    for built, stored in zip(case_inputs(tag), (logits, boxes, gt, present)):          # the fixture holds what the builders give
        assert torch.equal(built, stored)
    rec = decode_records_torch(logits, boxes, gt, present, K)
    assert rec["score"].dtype == torch.float32 and rec["iou"].dtype == torch.float32 and rec["box"].shape == (logits.shape[0], K, 6)
    check_records(rec, golden_records(g14, tag), "g14.torch")
    assert bool((rec["iou"][~present] == -1.0).all()) and bool((rec["iou"][present] >= 0.0).all())
    _check_metrics(_metrics({k: v.numpy() for k, v in rec.items()}), golden_metrics(g14, tag, "sparse"), tag)
    # through the record buffers, in ragged batches, with the golden records themselves as well
    buf = DetectionRecords(16, K, 0, "cpu")
    for lo, hi in ((0, 3), (3, 4), (4, logits.shape[0])):
        buf.append(logits[lo:hi], boxes[lo:hi], gt[lo:hi], present[lo:hi])
    host = buf.to_host()
    assert host["count"] == logits.shape[0] and host["score"].shape == (logits.shape[0], K)
    for name in ("score", "iou", "has_gt", "query", "box"):
        assert np.array_equal(host[name], rec[name].numpy()), name
    _check_metrics(_metrics(golden_records(g14, tag)), golden_metrics(g14, tag, "sparse"), tag + ".records")


@pytest.mark.parametrize("tag", CASES)
def test_complete_only_and_per_class_keys(g14, tag):
    rec = golden_records(g14, tag)
    _check_metrics(_metrics(rec, complete_only=True), golden_metrics(g14, tag, "complete"), tag + ".complete")
    full = golden_metrics(g14, tag, "full")
    assert "mAP_coco_liver_" in full and "AP_IoU_0.50_left_rectus_abdominis_" in full and "mAP_nndet_spleen_" in full
    _check_metrics(_metrics(rec, per_class=True), full, tag + ".full")


def test_metric_details():
    from transoar_amd.evaluation import detection_metrics, iou_thresholds, precision_table
    assert iou_thresholds().tolist() == [round(0.1 + 0.05 * i, 2) for i in range(18)]
    none = detection_metrics(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), ["a", "b", "c"], {1: "a"}, {2: "b"}, {"3": "c"})
    assert none["mAP_coco"] == 0.0 and none["AP_IoU_0.10"] == 0.0 and none["mAP_nndet_l"] == 0.0
    # a class without ground truth keeps precision 0; its detections are false positives of nobody else
    score = np.array([[0.9, 0.8], [0.7, 0.6]], np.float32)
    iou = np.array([[0.8, -1.0], [0.3, -1.0]], np.float32)
    has = np.array([[1, 0], [1, 0]], np.uint8)
    table = precision_table(score, iou, has)
    assert table.shape == (18, 101, 2) and float(table[:, :, 1].max()) == 0.0
    assert float(table[0, :, 0].min()) == 1.0 and float(table[17, :, 0].max()) == 0.0          # t = 0.1: both match; 0.95: none
    got = detection_metrics(score, iou, has, ["a", "b"], {1: "a"}, {2: "b"}, {})
    assert got["mAP_coco_m"] == 0.0 and np.isnan(got["mAP_coco_l"]) and got["AP_IoU_0.10"] == 0.5
    with pytest.raises(ValueError, match="classes"):
        detection_metrics(score, iou, has, ["a"])


# ---- 2. the record buffers ---------------------------------------------------------------------------------------------------
def test_overflow_raises_and_writes_nothing():
    from transoar_amd.evaluation import DetectionRecords, RecordsOverflow
    logits, boxes, gt, present = random_inputs(3, 4, 5, seed=1)
    losses = torch.tensor([1.0, 2.0])
    buf = DetectionRecords(5, 4, 2, "cpu")
    buf.append(logits, boxes, gt, present, losses)
    kept = {name: getattr(buf, name).clone() for name in ("score", "iou", "has_gt", "query", "box", "loss_sums")}
    assert buf.state.tolist() == [3, 0] and buf.to_host()["count"] == 3
    buf.append(logits, boxes, gt, present, losses)                      # 3 + 3 > 5
    assert buf.state.tolist() == [3, 1]
    for name, was in kept.items():
        assert torch.equal(getattr(buf, name), was), name
    with pytest.raises(RecordsOverflow, match="capacity"):
        buf.to_host()
    buf.append(logits[:2], boxes[:2], gt[:2], present[:2], losses)       # the flag stays, whatever fits later
    assert buf.state.tolist() == [5, 1]
    buf.reset()
    assert buf.state.tolist() == [0, 0] and float(buf.loss_sums.sum()) == 0.0
    buf.append(logits[:2], boxes[:2], gt[:2], present[:2], losses)
    buf.append(logits, boxes, gt, present, losses)                      # fills the capacity exactly
    host = buf.to_host()
    assert host["count"] == 5 and host["loss_sums"].tolist() == [2.0, 4.0]
    assert np.array_equal(host["score"][2:], kept["score"][:3].numpy())
    tiny = DetectionRecords(2, 4, 0, "cpu")
    tiny.append(logits, boxes, gt, present)                             # a batch larger than the whole buffer
    assert tiny.state.tolist() == [0, 1]
    with pytest.raises(ValueError, match="logits"):
        buf.append(logits[:, :19], boxes[:, :19], gt, present)
    with pytest.raises(ValueError, match="losses"):
        buf.append(logits, boxes, gt, present, torch.zeros(3))


def test_ties_and_nan_in_the_torch_path():
    from transoar_amd.evaluation import decode_records_torch
    logits = torch.tensor([0.5, 2.0, float("nan"), 2.0, -1.0, float("nan"), float("nan"), float("nan")]).reshape(1, 8, 1)
    boxes = torch.rand(1, 8, 6, generator=torch.Generator().manual_seed(0))
    rec = decode_records_torch(logits, boxes, torch.zeros(1, 2, 6), torch.zeros(1, 2, dtype=torch.bool), 2)
    assert rec["query"].tolist() == [[1, 0]]                            # the first of two equals; a number over a NaN
    assert torch.equal(rec["box"][0, 0], boxes[0, 1]) and torch.equal(rec["box"][0, 1], boxes[0, 4])
    rec = decode_records_torch(logits[:, 4:], boxes[:, 4:], torch.zeros(1, 4, 6), torch.zeros(1, 4, dtype=torch.bool), 4)
    assert rec["query"].tolist() == [[0, 0, 0, 0]] and bool(torch.isnan(rec["score"][0, 1:]).all())


# ---- 3. the C ABI: argument errors, no launch --------------------------------------------------------------------------------
def test_deteval_argument_errors():
    from transoar_amd.evaluation import lib          # bound from include/transoar_deteval.h
    f = lib.transoar_deteval_accumulate
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    F32, BF16, F16 = 0, 2, 3
    assert lib.transoar_deteval_abi_version() == 1

    def call(logits=p, boxes=p, dtype=F32, gt=p, present=p, losses=p, n_losses=2, n=2, k=20, qpo=27, state=p, capacity=8,
             score=p, iou=p, has=p, query=p, box=p, sums=p):
        return f(logits, boxes, dtype, gt, present, losses, n_losses, n, k, qpo, state, capacity, score, iou, has, query, box, sums,
                 None)
    for name in ("logits", "boxes", "gt", "present", "state", "score", "iou", "has", "query", "box"):
        assert call(**{name: None}) == -1, name
    assert call(sums=None) == -1                                   # losses given: the sums are required
    for bad in (dict(k=0), dict(k=65), dict(qpo=0), dict(qpo=4097), dict(n=0), dict(n=1025), dict(n_losses=-1), dict(n_losses=33),
                dict(capacity=0), dict(capacity=(1 << 20) + 1)):
        assert call(**bad) == -2, bad
    for dtype in (1, 4, -1):                                        # fp64 and unknown codes
        assert call(dtype=dtype) == -3
    assert call(logits=p + 2) == -4 and call(boxes=p + 1, dtype=BF16) == -4 and call(logits=p + 1, dtype=F16) == -4
    assert call(gt=p + 2) == -4 and call(state=p + 2) == -4 and call(sums=p + 4) == -4 and call(query=p + 1) == -4


# ---- 4. the Validator on a reduced-width model -------------------------------------------------------------------------------
@pytest.fixture
def _small_volume_masks():
    """The Focused Decoder's mask table only knows the dataset geometries: a test-only entry for the small volume."""
    from transoar_amd import focused_decoder
    saved = dict(focused_decoder._LEVEL_SHAPES)
    focused_decoder._LEVEL_SHAPES[20] = {"P%d" % k: tuple(max(v >> k, 1) for v in VOLUME) for k in range(6)}
    yield
    focused_decoder._LEVEL_SHAPES.clear()
    focused_decoder._LEVEL_SHAPES.update(saved)


def _small_model(seed=0):
    from tests._inputs import small_model_config
    from transoar_amd.transoarnet import TransoarNet, build_criterion
    cfg = small_model_config(False, use_cuda=False)
    torch.manual_seed(seed)
    net = TransoarNet(cfg)
    with torch.no_grad():                       # the heads start at zero in the reference: every query alike
        for prm in net.parameters():
            if prm.dim() > 1 and float(prm.abs().max()) == 0:
                torch.nn.init.xavier_uniform_(prm)
    return cfg, net, build_criterion(cfg)


def _validator(cfg, net, crit, **kw):
    from transoar_amd.evaluation import Validator
    return Validator(net, crit, cfg, classes=CLASSES, classes_small=subset(SMALL), classes_mid=subset(MID),
                     classes_large=subset(LARGE), amp_dtype=None, **kw)


def test_validator_on_the_reduced_model(_small_volume_masks):
    from tests._seg_inputs import paint_labels
    from transoar_amd.box_targets import targets_from_labels
    from transoar_amd.config import synthetic_targets
    from transoar_amd.evaluation import decode_records_torch
    torch.set_num_threads(8)
    cfg, net, crit = _small_model()
    val = _validator(cfg, net, crit, capacity=8)
    with pytest.raises(RuntimeError, match="nothing was added"):
        val.compute()
    x = torch.rand(2, 1, *VOLUME, generator=torch.Generator().manual_seed(2))
    labels = paint_labels(synthetic_targets(2, 20, seed=1), VOLUME)
    dense = targets_from_labels(labels, 20, cfg["bbox_padding"])
    assert 0 < int(dense.present.sum()) < 40            # some boxes are thinner than the reference's minimum of 5 voxels
    net.train()
    out, losses = val.add(x, None, labels)                # targets=None: from the label volume
    assert net.training, "add() restores the mode it found"
    assert not out["pred_logits"].requires_grad
    net.eval()
    val.add(x, [{"boxes": dense.boxes[i][dense.present[i]], "labels": torch.nonzero(dense.present[i])[:, 0] + 1} for i in (0, 1)])
    assert not net.training
    with torch.no_grad():
        want = net(x)
        want_losses = crit(want, dense, None, net._anchors)
    assert torch.equal(out["pred_logits"], want["pred_logits"]), "add() runs the model in eval mode (no dropout)"
    rec = decode_records_torch(want["pred_logits"], want["pred_boxes"], dense.boxes, dense.present, 20)
    host = val.records.to_host()
    assert host["count"] == 4
    for name in ("score", "iou", "has_gt", "query", "box"):
        assert np.array_equal(host[name][:2], rec[name].numpy()), name
        assert np.array_equal(host[name][2:], rec[name].numpy()), name          # the same batch, its targets as a list
    preds = val.predictions()
    assert len(preds) == 4 and preds[0][0].shape == (20, 6) and preds[0][1].tolist() == list(range(1, 21))
    assert np.array_equal(preds[1][2], rec["score"][1].numpy())
    metrics = val.compute()
    ref = _metrics({k: np.concatenate((v.numpy(), v.numpy())) for k, v in rec.items()})
    for name, value in ref.items():
        assert metrics[name] == value, name
    coefs = cfg["loss_coefs"]
    total = sum(float(v) * coefs[k.split("_")[0]] for k, v in want_losses.items())
    assert list(metrics)[len(ref):] == ["loss/total"] + ["loss/" + k for k in want_losses]
    for k, v in want_losses.items():
        assert abs(metrics["loss/" + k] - float(v)) <= 1e-5 * max(abs(float(v)), 1.0), k
    assert abs(metrics["loss/total"] - total) <= 1e-5 * abs(total)
    # the reference's >= rule, and what save_checkpoint is given
    assert val.metric_max_val == 0.0 and val.is_best({"mAP_coco": 0.0}) and val.is_best({"mAP_coco": 0.25})
    assert val.metric_max_val == 0.25 and not val.is_best({"mAP_coco": 0.2}) and val.is_best({"mAP_coco": 0.25})
    val.reset()
    assert val.records.to_host()["count"] == 0
    # outputs the caller already has, without losses: a pass of its own
    bare = _validator(cfg, net, crit, capacity=2)
    bare.add_outputs(want, dense)
    assert bare.compute() == {k: v for k, v in _metrics({k: v.numpy() for k, v in rec.items()}).items()}
    bare.add_outputs(want, dense)
    with pytest.raises(RuntimeError, match="capacity"):
        bare.compute()
    with pytest.raises(ValueError, match="seg_targets"):
        val.add(x, None)


# ---- 5. two ranks ------------------------------------------------------------------------------------------------------------
class _NoModel(torch.nn.Module):
    _anchors = None


def _rank_batches(tag, rank):
    """Rank r holds images r, r + 2, ... of the case, in two batches."""
    logits, boxes, gt, present = case_inputs(tag)
    idx = torch.arange(rank, logits.shape[0], 2)
    return [tuple(t[idx[lo:hi]].contiguous() for t in (logits, boxes, gt, present)) for lo, hi in ((0, 2), (2, len(idx)))]


def _feed(val, batches, base):
    from transoar_amd.matcher import DenseTargets
    for i, (logits, boxes, gt, present) in enumerate(batches):
        losses = {"bbox": torch.tensor(base + i), "cls": torch.tensor(2.0 * base)}
        val.add_outputs({"pred_logits": logits, "pred_boxes": boxes}, DenseTargets(gt, present, int(present.sum())), losses)


def _bare_validator():
    from transoar_amd.evaluation import Validator
    cfg = {"num_classes": K, "loss_coefs": {"bbox": 5, "cls": 2}}
    return Validator(_NoModel(), None, cfg, classes=CLASSES, classes_small=subset(SMALL), classes_mid=subset(MID),
                     classes_large=subset(LARGE), capacity=16)


def _gloo_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    val = _bare_validator()
    _feed(val, _rank_batches("ties", rank), 1.0 + rank)
    metrics = val.compute(process_group=dist.group.WORLD, per_class=True)
    if rank == 1:
        torch.save(metrics, out_path)
    dist.destroy_process_group()


def test_two_ranks_equal_one_fed_rank_major():
    """Tied scores keep insertion order, so the order of the gather is part of the contract: rank-major."""
    one = _bare_validator()
    _feed(one, _rank_batches("ties", 0), 1.0)
    _feed(one, _rank_batches("ties", 1), 2.0)
    want = one.compute(per_class=True)
    other = _bare_validator()                       # the same images in their original order: ties fall differently
    _feed(other, [case_inputs("ties")], 1.0)
    assert any(other.compute(per_class=True)[k] != v for k, v in want.items() if not k.startswith("loss/"))
    with tempfile.TemporaryDirectory() as tmp:
        out_path = os.path.join(tmp, "out.pt")
        mp.spawn(_gloo_worker, args=(2, 29500 + (os.getpid() % 2000), out_path), nprocs=2, join=True)
        got = torch.load(out_path)
    assert list(got) == list(want)
    for name, value in want.items():
        assert got[name] == value, (name, got[name], value)
    assert want["loss/bbox"] == (1.0 + 2.0 + 2.0 + 3.0) / 4 and want["loss/cls"] == 3.0
    assert want["loss/total"] == 5 * want["loss/bbox"] + 2 * want["loss/cls"]


# ---- 6. the fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference")
def test_fixture_regenerates_identically(g14):
    spec = importlib.util.spec_from_file_location("_make_golden_eval", os.path.join(ROOT, "tests", "golden", "make_golden_eval.py"))
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
    assert sorted(store) == sorted(g14.files)
    for name, arr in store.items():
        assert arr.dtype == g14[name].dtype and arr.shape == g14[name].shape and np.array_equal(arr, g14[name]), name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_detection_eval.npz")) < 100 * 1024
