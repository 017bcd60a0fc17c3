#!/usr/bin/env python
"""Generate tests/golden/g14_detection_eval.npz (detection validation) by IMPORTING THE REFERENCE, as make_golden_boxes.py does
for g13: runs only where the reference is available, on the CPU; the GPU box only sees the .npz.

For every case of tests/_eval_inputs.py::CASES: the inputs (fp32 logits, boxes, ground truth), per (image, class) the query
the reference's inference() decodes, its score and its IoU with the class's ground truth (iou_3d_np; -1 without one), and every
metric of a DetectionEvaluator (coco (0.5, 0.95, 0.05), nnDet (0.1, 0.5, 0.05)) over the images: with sparse_results=True
("sparse"), with sparse_results=False ("full": the per-class keys too) and over only the images that have every class
("complete", scripts/test.py:97).  inference() returns from inside its batch loop, so it is called one sample at a time.

The generator asserts what keeps the reference alone within the tests' bounds: every IoU at least 1e-4 away from every threshold,
the two largest probabilities of an organ at least 1e-5 apart, and any two scores of one class at least 1e-5 apart or -- only in
the case that ties on purpose -- from identical logits.

    python tests/golden/make_golden_eval.py
"""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _evaluate(evaluator_cls, inference, images, logits, boxes, gt, present, sparse):
    from tests._eval_inputs import CLASSES, K, LARGE, MID, SMALL, subset
    ev = evaluator_cls(classes=list(CLASSES), classes_small=subset(SMALL), classes_mid=subset(MID), classes_large=subset(LARGE),
                       iou_range_nndet=(0.1, 0.5, 0.05), iou_range_coco=(0.5, 0.95, 0.05), sparse_results=sparse)
    for i in images:
        pred_boxes, pred_classes, pred_scores = inference({"pred_logits": logits[i:i + 1], "pred_boxes": boxes[i:i + 1]}, K)
        ids = np.nonzero(present[i].numpy())[0] + 1
        ev.add(pred_boxes=pred_boxes, pred_classes=pred_classes, pred_scores=pred_scores,
               gt_boxes=[gt[i][present[i]].numpy().reshape(-1, 6)], gt_classes=[ids])
    return ev.eval()


def arrays():
    """-> {name: array} of the fixture"""
    for p in (REF, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tests._eval_inputs import CASES, CLASSES, K, LARGE, MID, QPO, SMALL, case_inputs
    from transoar.evaluator import DetectionEvaluator
    from transoar.inference import inference
    from transoar.utils.bboxes import iou_3d_np
    store = {"classes": np.array(CLASSES), "classes_small": np.array(SMALL), "classes_mid": np.array(MID),
             "classes_large": np.array(LARGE)}
    thresholds = np.round(np.arange(18) * 0.05 + 0.1, 2)
    for tag in CASES:
        logits, boxes, gt, present = case_inputs(tag)
        m = logits.shape[0]
        query = np.zeros((m, K), np.int32)
        score = np.zeros((m, K), np.float32)
        iou = np.full((m, K), -1.0, np.float32)
        for i in range(m):
            pred_boxes, pred_classes, pred_scores = inference({"pred_logits": logits[i:i + 1], "pred_boxes": boxes[i:i + 1]}, K)
            assert pred_classes[0].tolist() == list(range(1, K + 1))
            probs = logits[i:i + 1].sigmoid().squeeze().reshape(1, K, QPO)          # inference.py:10-12
            query[i] = probs.argmax(dim=-1)[0].numpy()
            score[i] = pred_scores[0]
            for c in range(K):
                assert np.array_equal(pred_boxes[0][c], boxes[i, c * QPO + query[i, c]].numpy())
                if present[i, c]:
                    iou[i, c] = iou_3d_np(pred_boxes[0][c][None], gt[i, c].numpy()[None])[0, 0]
            top = np.sort(probs[0].double().numpy(), -1)
            assert (top[:, -1] - top[:, -2]).min() >= 1e-5, tag
        has = present.numpy()
        assert np.abs(iou[has][:, None].astype(np.float64) - thresholds[None]).min(initial=1.0) >= 1e-4, tag
        win = logits.reshape(m, K, QPO).amax(-1).numpy()
        for c in range(K):
            gap = np.abs(score[:, None, c].astype(np.float64) - score[None, :, c])
            same = win[:, None, c] == win[None, :, c]
            assert (gap[~same] >= 1e-5).all(), tag
            assert tag == "ties" or same.sum() == m, tag
        if tag == "ties":
            assert all(len(set(win[:, c].tolist())) < m for c in range(K))
        complete = [i for i in range(m) if bool(present[i].all())]
        results = {"sparse": _evaluate(DetectionEvaluator, inference, range(m), logits, boxes, gt, present, True),
                   "full": _evaluate(DetectionEvaluator, inference, range(m), logits, boxes, gt, present, False),
                   "complete": _evaluate(DetectionEvaluator, inference, complete, logits, boxes, gt, present, True)}
        store.update({"%s.logits" % tag: logits.numpy(), "%s.boxes" % tag: boxes.numpy(), "%s.gt_boxes" % tag: gt.numpy(),
                      "%s.gt_present" % tag: has, "%s.query" % tag: query, "%s.score" % tag: score, "%s.iou" % tag: iou})
        for which, res in results.items():
            names = "names_full" if which == "full" else "names_sparse"        # the same keys in every case: stored once
            assert store.setdefault(names, np.array(list(res))).tolist() == list(res)
            store["%s.%s_values" % (tag, which)] = np.array([float(res[key]) for key in res], np.float64)
    return store


if __name__ == "__main__":
    store = arrays()
    for name in sorted(store):
        if name.endswith(".sparse_values"):
            print(name, np.round(store[name], 4).tolist())
    path = os.path.join(HERE, "g14_detection_eval.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path))
