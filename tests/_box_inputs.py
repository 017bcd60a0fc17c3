"""Inputs of the box-target tests (transoar_amd/box_targets.py), shared with tests/golden/make_golden_boxes.py."""
import torch

NUM_CLASSES = 20
PADDINGS = (0, 1, 3)
# every box value lies in [0, 1] and is the result of at most three correctly rounded fp32 operations on exact integers
BOX_TOL = 2.0 ** -22

# g13: tag -> (shape (N, D, H, W), [(sample, class, (x0, x1), (y0, y1), (z0, z1)) painted in order, half-open ranges])
CASES = {
    # uint8: sample 1 starts at byte 15470 (not a multiple of 16); rows of 70 are no multiple of a 16-byte group
    "A": ((2, 13, 17, 70), [
        (0, 1, (0, 1), (0, 1), (0, 1)), (0, 1, (12, 13), (16, 17), (69, 70)),      # two isolated voxels: the whole volume
        (0, 2, (2, 9), (3, 10), (10, 15)),                                          # z extent 4: dropped
        (0, 3, (2, 9), (3, 10), (20, 26)),                                          # z extent 5: kept
        (0, 4, (1, 4), (1, 4), (30, 33)), (0, 4, (8, 12), (10, 15), (50, 60)),      # two blobs, one box
        (1, 5, (3, 10), (2, 12), (5, 40)),
        (1, 3, (0, 6), (0, 6), (60, 70)),
    ]),
    # 30 workgroups per sample; class 3 only in the first and the last voxel of the volume
    "B": ((1, 40, 48, 64), [
        (0, 3, (0, 1), (0, 1), (0, 1)), (0, 3, (39, 40), (47, 48), (63, 64)),
        (0, 7, (15, 25), (18, 30), (20, 44)),
    ]),
    # aligned; sample 1 is background only
    "C": ((3, 16, 16, 64), [
        (0, 1, (2, 10), (3, 12), (5, 30)), (0, 20, (8, 16), (0, 16), (40, 64)),
        (2, 2, (0, 8), (0, 8), (0, 8)), (2, 9, (5, 9), (5, 12), (10, 20)),          # class 9: x extent 3, dropped
    ]),
    # one voxel: the reference returns empty tensors
    "D": ((1, 8, 8, 8), [(0, 7, (3, 4), (4, 5), (5, 6))]),
}


def case_labels(tag):
    """-> uint8 (N, D, H, W)"""
    shape, paint = CASES[tag]
    vol = torch.zeros(shape, dtype=torch.uint8)
    for s, c, (x0, x1), (y0, y1), (z0, z1) in paint:
        vol[s, x0:x1, y0:y1, z0:z1] = c
    return vol


def dense_from_reference(boxes, classes, n, k=NUM_CLASSES):
    """The reference's per-sample (boxes (M, 6), classes (M,)) -> dense boxes (N, k, 6) fp32 and present (N, k) bool."""
    dense = torch.zeros(n, k, 6)
    present = torch.zeros(n, k, dtype=torch.bool)
    for s in range(n):
        cls = torch.as_tensor(classes[s]).long().reshape(-1)
        if cls.numel():
            dense[s, cls - 1] = torch.as_tensor(boxes[s]).float().reshape(-1, 6)
            present[s, cls - 1] = True
    return dense, present


def check_targets(got, ref_boxes, ref_present, key):
    """got: DenseTargets against dense reference boxes (N, k, 6) fp32 / present (N, k) bool: present exact, boxes within BOX_TOL
    and (same operations in the same order in IEEE fp32) bit-identical, absent rows zero, both counts = number of boxes."""
    from tests._observe import observe
    ref_boxes, ref_present = ref_boxes.detach().float().cpu(), ref_present.detach().cpu()
    assert got.present.dtype == torch.bool and torch.equal(got.present.cpu(), ref_present)
    mine = got.boxes.detach().cpu()
    assert mine.dtype == torch.float32 and mine.shape == ref_boxes.shape
    differ = observe(key + ".bits_differ", float((mine.view(torch.int32) != ref_boxes.view(torch.int32)).sum()), 0)
    err = observe(key + ".abs", float((mine - ref_boxes).abs().max()), BOX_TOL)
    assert err <= BOX_TOL, err
    assert differ == 0, "bit-identical boxes expected, %d values differ" % differ
    assert float(mine[~ref_present].abs().sum()) == 0.0, "absent rows are all zero"
    count = int(ref_present.sum())
    assert torch.is_tensor(got.num_boxes) and torch.is_tensor(got.n_present)
    assert float(got.num_boxes) == count and float(got.n_present) == count


def golden_case(g13, tag, padding):
    """-> (labels uint8 (N, D, H, W), per-sample boxes, per-sample classes) of the fixture"""
    labels = torch.from_numpy(g13["%s.labels" % tag])
    n = labels.shape[0]
    boxes = [torch.from_numpy(g13["%s.p%d.boxes.%d" % (tag, padding, s)]) for s in range(n)]
    classes = [torch.from_numpy(g13["%s.p%d.classes.%d" % (tag, padding, s)]) for s in range(n)]
    return labels, boxes, classes


def blob_volume(shape, k, dtype, seed):
    """(N, D, H, W) of `dtype`: per sample 6-10 axis-aligned blobs of random classes in 1..k and 20 isolated voxels, then labels the
    targets must ignore sprinkled in: k + 1 and, for signed types, -1."""
    g = torch.Generator().manual_seed(seed)

    def r(lo, hi):
        return int(torch.randint(lo, hi, (1,), generator=g))
    n, dims = shape[0], shape[1:]
    vol = torch.zeros(shape, dtype=torch.int64)
    for s in range(n):
        for _ in range(r(6, 11)):
            lo = [r(0, d) for d in dims]
            hi = [min(d, l + 1 + r(0, max(2, d // 2))) for l, d in zip(lo, dims)]
            vol[s, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = r(1, k + 1)
        for i in range(40):
            pos = tuple(r(0, d) for d in dims)
            vol[(s,) + pos] = r(1, k + 1) if i < 20 else (k + 1 if i % 2 or not dtype.is_signed else -1)
    return vol.to(dtype)
