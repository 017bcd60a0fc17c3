"""Inputs of the detection-validation tests (transoar_amd/evaluation.py), shared with tests/golden/make_golden_eval.py."""
import numpy as np
import torch

K, QPO, IMAGES = 20, 27, 10
# a sigmoid probability lies in [0, 1]; two correctly rounded fp32 evaluations of 1 / (1 + exp(-x)) with exp within one unit in
# the last place each stay within 2^-23 of the true value: the project's fp32 bound for values in [0, 1] (tests/_box_inputs.py)
SCORE_TOL = 2.0 ** -22
METRIC_TOL = 1e-12

# class names and small / mid / large subsets of the reference's config/visceral.yaml
CLASSES = ["liver", "spleen", "pancreas", "gall_bladder", "urinary_bladder", "aorta", "trachea", "right_lung", "left_lung",
           "sternum", "thyroid_gland", "first_lumbar_vertebra", "right_kidney", "left_kidney", "right_adrenal_gland",
           "left_adrenal_gland", "right_psoas_major", "left_psoas_major", "right_rectus_abdominis", "left_rectus_abdominis"]
SMALL, MID, LARGE = (3, 4, 5, 7, 11, 12, 15, 16), (2, 6, 10, 13, 14, 17, 18, 19, 20), (1, 8, 9)

CASES = ("generic", "absent_some", "absent_class", "ties", "no_gt_image", "perfect", "disjoint")
# per case the first seed from 1400 + 10 * its index at which every IoU stays 1e-4 away from every threshold (the values sit on a
# grid, so an IoU can be a threshold exactly; make_golden_eval.py asserts the margin on the reference's own IoUs)
SEEDS = {"generic": 1400, "absent_some": 1410, "absent_class": 1423, "ties": 1430, "no_gt_image": 1441, "perfect": 1450,
         "disjoint": 1460}
ABSENT_CLASS = 5           # 1-based: no image of "absent_class" has it
NO_GT_IMAGE = 3             # the image of "no_gt_image" without any ground truth


def subset(ids):
    """-> {class id: name}, the form the reference's config has"""
    return {int(i): CLASSES[int(i) - 1] for i in ids}


def case_inputs(tag, seed=None):
    """-> logits (M, K * QPO, 1), boxes (M, K * QPO, 6), gt_boxes (M, K, 6) fp32 and gt_present (M, K) bool, M = IMAGES.

    Every value sits on a coarse binary grid (boxes: multiples of 2^-7, logits: multiples of 1/4), so that the fixture stays
    small.  Per (image, class) one query wins by at least 1/4 in the logit; the winners of one class have distinct logits
    across the images, except in "ties", where images share them.  All other queries of a class carry the class's anchor box."""
    g = torch.Generator().manual_seed(SEEDS[tag] if seed is None else seed)

    def grid(lo, hi, *shape):          # multiples of 2^-7 in [lo, hi]
        return torch.randint(int(round(lo * 128)), int(round(hi * 128)) + 1, shape, generator=g).float() / 128

    m = IMAGES
    gt = torch.cat((grid(0.3, 0.7, m, K, 3), grid(0.1, 0.2, m, K, 3)), -1)
    present = torch.ones(m, K, dtype=torch.bool)
    if tag in ("absent_some", "absent_class"):
        present = torch.rand(m, K, generator=g) < 0.7
        present[0] = True                                          # one complete image
    if tag == "absent_class":
        present[:, ABSENT_CLASS - 1] = False
    if tag == "no_gt_image":
        present[NO_GT_IMAGE] = False
    gt = torch.where(present[:, :, None], gt, torch.zeros_like(gt))
    # the winner's box: the ground truth moved and resized (where there is none: a box of its own)
    own = torch.cat((grid(0.3, 0.7, m, K, 3), grid(0.1, 0.2, m, K, 3)), -1)
    base = torch.where(present[:, :, None], gt, own)
    shift = torch.cat((grid(-0.04, 0.04, m, K, 3), grid(-0.02, 0.02, m, K, 3)), -1)
    shift[::2] = (shift[::2] * (128 / 3)).round() / 128              # every other image: a third of the offset
    if tag == "perfect":
        shift = torch.zeros_like(shift)
    if tag == "disjoint":
        shift = torch.cat((torch.full((m, K, 3), 0.25), torch.zeros(m, K, 3)), -1)      # 0.25 > the largest size 0.2
    win_box = base + shift
    anchors = torch.cat((grid(0.3, 0.7, K, 3), grid(0.1, 0.2, K, 3)), -1)
    boxes = anchors[None, :, None, :].repeat(m, 1, QPO, 1)
    # winners: per class a permutation of m distinct logit levels (scores of one class differ); "ties": only m // 3 levels
    levels = torch.stack([torch.randperm(m, generator=g) for _ in range(K)], 1)          # (m, K)
    if tag == "ties":
        levels = levels // 3
    win_logit = -1.0 + 0.25 * levels.float()
    # the rest: a fixed low pattern (it compresses to nothing), but three runners-up per organ 1/4 .. 2 below the winner
    j = torch.arange(QPO)[None, None, :]
    logits = (-3.5 - 0.25 * ((3 * j + torch.arange(K)[None, :, None]) % 8).float()).repeat(m, 1, 1)
    for _ in range(3):
        at = torch.randint(0, QPO, (m, K, 1), generator=g)
        logits.scatter_(2, at, win_logit[:, :, None] - 0.25 * (1 + torch.randint(0, 8, (m, K, 1), generator=g)).float())
    slot = torch.randint(0, QPO, (m, K), generator=g)
    logits.scatter_(2, slot[:, :, None], win_logit[:, :, None])
    boxes.scatter_(2, slot[:, :, None, None].expand(m, K, 1, 6), win_box[:, :, None, :])
    return logits.reshape(m, K * QPO, 1).contiguous(), boxes.reshape(m, K * QPO, 6).contiguous(), gt.contiguous(), present


def random_inputs(n, k, qpo, seed, dtype=torch.float32, ties=False):
    """Seeded random inputs of the kernel-against-torch tests: logits ~ 2 N(0, 1), boxes and ground truth with overlaps of every
    size, about a fifth of the classes absent; values rounded to `dtype` (returned in it; the ground truth stays fp32).
    ties: some organs get their largest logit twice more (the lowest index must win) and a NaN logit (which must not)."""
    g = torch.Generator().manual_seed(seed)
    logits = 2 * torch.randn(n, k, qpo, generator=g)
    if ties and qpo >= 4:
        top = logits.amax(-1)
        for s in range(n):
            for c in range(0, k, 2):
                at = torch.randperm(qpo, generator=g)[:3]
                logits[s, c, at[0]] = top[s, c]
                logits[s, c, at[1]] = top[s, c]
                logits[s, c, at[2]] = float("nan")
    gt = torch.cat((0.3 + 0.4 * torch.rand(n, k, 3, generator=g), 0.1 + 0.1 * torch.rand(n, k, 3, generator=g)), -1)
    present = torch.rand(n, k, generator=g) < 0.8
    gt = torch.where(present[:, :, None], gt, torch.zeros_like(gt))
    centre = gt[:, :, None, :3] + 0.1 * (torch.rand(n, k, qpo, 3, generator=g) - 0.5) + 0.4 * (~present)[:, :, None, None]
    size = 0.1 + 0.1 * torch.rand(n, k, qpo, 3, generator=g)
    boxes = torch.cat((centre, size), -1)
    return (logits.reshape(n, k * qpo, 1).to(dtype).contiguous(), boxes.reshape(n, k * qpo, 6).to(dtype).contiguous(),
            gt.contiguous(), present)


def top_two_gap(logits, k):
    """Smallest difference between the two largest DISTINCT-logit probabilities of an organ, in float64 (1.0 with one query)."""
    n, q = logits.shape[0], logits.shape[1]
    x = logits.reshape(n, k, q // k).double()
    x = torch.where(torch.isnan(x), torch.full_like(x, -1e9), x)
    p = torch.sigmoid(x)
    best = p.amax(-1, keepdim=True)
    rest = torch.where(x == x.amax(-1, keepdim=True), torch.full_like(p, -1.0), p).amax(-1, keepdim=True)
    gap = torch.where(rest < 0, torch.ones_like(best), best - rest)
    return float(gap.min())


def check_records(got, want, key):
    """got / want: dicts of (n, k) records (tensors or arrays).  query and has_gt exact, IoU bit-identical, score within SCORE_TOL
    (NaN where the other has NaN), boxes equal."""
    from tests._observe import observe

    def arr(v):
        return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    assert np.array_equal(arr(got["query"]).astype(np.int64), arr(want["query"]).astype(np.int64)), key
    assert np.array_equal(arr(got["has_gt"]) != 0, arr(want["has_gt"]) != 0), key
    a, b = arr(got["score"]).astype(np.float32), arr(want["score"]).astype(np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b)), key
    err = observe(key + ".score_abs", float(np.nanmax(np.abs(a - b), initial=0.0)), SCORE_TOL)
    assert err <= SCORE_TOL, (key, err)
    i, j = arr(got["iou"]).astype(np.float32), arr(want["iou"]).astype(np.float32)
    differ = observe(key + ".iou_bits_differ", float((i.view(np.int32) != j.view(np.int32)).sum()), 0)
    assert differ == 0, "%s: bit-identical IoU expected, %d values differ (max %g)" % (key, differ, np.abs(i - j).max())
    if "box" in got and "box" in want:
        assert np.array_equal(arr(got["box"]).astype(np.float32).view(np.int32), arr(want["box"]).astype(np.float32).view(np.int32)), key
    return err


def golden_records(g14, tag):
    rec = {name: g14["%s.%s" % (tag, name)] for name in ("query", "score", "iou")}
    rec["has_gt"] = g14["%s.gt_present" % tag]
    return rec


def golden_metrics(g14, tag, which):
    """which: "sparse", "full" (per class) or "complete" (only the images with every class) -> {key: value}"""
    names = g14["names_full" if which == "full" else "names_sparse"]
    return dict(zip((str(s) for s in names), g14["%s.%s_values" % (tag, which)].tolist()))
