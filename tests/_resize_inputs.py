"""Inputs of the resize tests (transoar_amd/resize.py), seeded and shared: the two cases of the kernel tests with per-sample
windows, their fp64 restatements (computed once per process and never modified), and the toy configuration of TestSplit."""
import functools

import torch

N = 2
SHAPE = (30, 43, 57)
A_MIN, A_MAX = 0.1, 0.9            # neither is an fp32 number: every path rounds them to fp32 first
DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)

# tag -> (window rows (start, extent, crop) per sample, resized grid, out shape).  "trap": every axis of sample 0 is a pair on
# which the integer nearest rule o E // R differs from torch's fp32 rule (26 -> 22, 39 -> 33, 52 -> 22); sample 1 has another
# window (whose D axis, 13 -> 22, is upsampled).  "mixed": D is upsampled 5 -> 8 (bins of one and two voxels).  The crops are
# not zero and out is narrower than the resized grid on some axis.
CASES = {
    "trap": ((((2, 3, 4), (26, 39, 52), (0, 0, 0)), ((4, 0, 5), (13, 43, 52), (0, 0, 0))), (22, 33, 22), (22, 33, 22)),
    "trap_crop": ((((2, 3, 4), (26, 39, 52), (1, 2, 3)), ((4, 0, 5), (13, 43, 52), (0, 4, 1))), (22, 33, 22), (20, 29, 16)),
    "mixed": ((((2, 3, 4), (5, 39, 52), (0, 0, 0)), ((25, 4, 0), (5, 39, 52), (0, 0, 0))), (8, 33, 22), (8, 33, 22)),
    "mixed_crop": ((((2, 3, 4), (5, 39, 52), (2, 1, 0)), ((25, 4, 0), (5, 39, 52), (0, 3, 2))), (8, 33, 22), (6, 30, 19)),
}


def inputs(shape=SHAPE, n=N, seed=0):
    """image (n, *shape) fp32 = rand, labels (n, *shape) int64 = randint(0, 6)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, *shape, generator=g), torch.randint(0, 6, (n, *shape), generator=g)


def ct_inputs(shape=SHAPE, n=N, seed=1):
    """An int16 image as a CT file holds it (-1024 .. 3071) and the labels of inputs()."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 3072, (n, *shape), generator=g).to(torch.int16), inputs(shape, n)[1]


def window_table(rows):
    """rows of (start, extent, crop) -> the table (n, 12) int32 (found = 1)."""
    table = torch.zeros(len(rows), 12, dtype=torch.int32)
    for i, (start, extent, crop) in enumerate(rows):
        table[i, 0:3], table[i, 3:6], table[i, 6:9] = torch.tensor(start), torch.tensor(extent), torch.tensor(crop)
        table[i, 9] = 1
    return table


def case(tag):
    rows, resized, out = CASES[tag]
    return window_table(rows), resized, out


@functools.lru_cache(maxsize=None)
def reference(tag, scaled, ct=False):
    """-> (image, labels int64, table, resized, out, fp64 image, labels) of a case on the shared inputs; `scaled`: with range
    scaling (A_MIN / A_MAX on the fp32 image, -200 / 300 on the int16 one)."""
    from transoar_amd.resize import resize_torch
    image, labels = ct_inputs() if ct else inputs()
    table, resized, out = case(tag)
    lo, hi = (None, None) if not scaled else ((-200.0, 300.0) if ct else (A_MIN, A_MAX))
    ref, ref_lab = resize_torch(image, labels, table, resized, out, lo, hi, dtype=torch.float64)
    return image, labels, table, resized, out, ref, ref_lab, lo, hi


def tensor_max_normalised(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def integer_rule_differs(extent, resized):
    """Does o E // R differ from torch's fp32 nearest rule for some o?"""
    from transoar_amd.resize import nearest_index
    o = torch.arange(resized)
    return not torch.equal((o * extent) // resized, nearest_index(o, extent, resized))


def split_config(median, patch=None):
    """The keys TestSplit and BatchAugment read, on a toy volume (values of the shipped YAMLs where they matter)."""
    aug = dict(use_augmentation=True, patch_size=None if patch is None else list(patch), p_gaussian_noise=0, p_gaussian_smooth=0,
               p_intensity_scale=0.5, p_intensity_shift=0.5, p_adjust_contrast=0, p_rotate=0.5, p_zoom=0.5, p_shear=0.0,
               p_translate=0.5, p_flip=0, intensity_scale_factors=0.1, intensity_shift_offsets=0.1, rotation=[-15, 15],
               min_zoom=0.8, max_zoom=1.2, translate_precentage=10, flip_axis=[0, 1, 2])
    return dict(augmentation=aug, foreground_voxel_statistics=dict(percentile_00_5=A_MIN, percentile_99_5=A_MAX),
                shape_statistics=dict(median=list(median)))


def blobs(shape=SHAPE, n=N, empty=None):
    """A label map (n, *shape) int64 of a few boxes of classes 1, 3, 6, 14 and 40 (sample `empty`, if given, is all background)."""
    lab = torch.zeros(n, *shape, dtype=torch.int64)
    d, h, w = shape
    for s in range(n):
        if s == empty:
            continue
        k = s + 1
        lab[s, 5 + k:9 + k, 7:12 + k, 10 + k:20] = 1
        lab[s, 12:15, 20 + k:25 + k, 30:41 + k] = 3
        lab[s, d - 6 - k:d - 3, 14:16, 3 + k:6 + k] = 6
        lab[s, 9:11, h - 5 - k:h - 2, w - 9:w - 1 - k] = 14
        lab[s, 2 + k, 3, 4] = 40
    return lab
