#!/usr/bin/env python
"""Generate tests/golden/g13_box_targets.npz (detection targets from label volumes) by IMPORTING THE REFERENCE, as
make_golden_seg.py does for g12: runs only where the reference is available, on the CPU; the GPU box only sees the .npz.

For every case of tests/_box_inputs.py::CASES the label volume (uint8) and, for every padding of PADDINGS, what the reference's
segmentation2bbox(labels (N, 1, D, H, W), padding, 'cxcyczwhd', normalize=True) (transoar/utils/bboxes.py:45-96) returns per
sample: boxes (M, 6) fp32 and classes (M,) int64, M = 0 where it returns empty tensors.

    python tests/golden/make_golden_boxes.py
"""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def arrays():
    """-> {name: array} of the fixture"""
    for p in (REF, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tests._box_inputs import CASES, PADDINGS, case_labels
    from transoar.utils.bboxes import segmentation2bbox
    store = {}
    for tag in CASES:
        labels = case_labels(tag)
        store["%s.labels" % tag] = labels.numpy()
        for padding in PADDINGS:
            boxes, classes = segmentation2bbox(labels[:, None].long(), padding, "cxcyczwhd", normalize=True)
            for s, (b, c) in enumerate(zip(boxes, classes)):
                store["%s.p%d.boxes.%d" % (tag, padding, s)] = b.float().reshape(-1, 6).numpy()
                store["%s.p%d.classes.%d" % (tag, padding, s)] = c.long().reshape(-1).numpy()
    return store


if __name__ == "__main__":
    store = arrays()
    for name in sorted(store):
        if ".classes." in name:
            print(name, store[name].tolist())
    path = os.path.join(HERE, "g13_box_targets.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path))
