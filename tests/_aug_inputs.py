"""Inputs of the augmentation tests (transoar_amd/augment.py): the four maps of the kernel tests, their tables, and the fp64
restatement of each case, computed once per process and never modified."""
import functools

import torch

IN_SHAPE = (24, 20, 36)
N = 2
A_MIN, A_MAX = 0.1, 0.9            # neither is an fp32 number: every path rounds them to fp32 first
DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)
BAND = 1e-3                        # |frac(src) - 0.5| below this on some axis: a near-tie of the nearest-label rule

# tag -> (angles in degrees about (D, H, W), divisor, flip signs, t, out shape, gain, offset):  M = Rx Ry Rz diag(signs) / divisor and
# src = c + M (o + crop - c) + t  with c the input centre and crop the centred window's offset (t BEFORE the centres are folded in).
MAPS = {
    "shipped": ((4.3, -3.1, 4.9), 1.07, (1, 1, 1), (1.7, -1.3, 2.9), IN_SHAPE, 1.07, -0.04),
    "zoomout": ((0.0, 0.0, -5.0), 0.91, (1, 1, 1), (-2.2, 0.6, -3.4), IN_SHAPE, 0.93, 0.06),
    "crop": ((0.0, 2.0, 0.0), 1.1, (1, 1, 1), (3.3, -2.1, 4.7), (16, 12, 20), 1.0, 0.0),
    "exact": ((0.0, 0.0, 0.0), 1.0, (-1, 1, -1), (2.0, -3.0, 5.0), IN_SHAPE, 1.0, 0.0),
}


def inputs(shape=IN_SHAPE, n=N, seed=0):
    """image (n, *shape) fp32 = rand, labels (n, *shape) int64 = randint(0, 6)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, *shape, generator=g), torch.randint(0, 6, (n, *shape), generator=g)


def raw_table(m, t, in_shape, out_shape, gain=1.0, offset=0.0):
    """One table row from M (3 x 3) and t as MAPS states them, folded in fp64 and rounded once."""
    m = torch.as_tensor(m, dtype=torch.float64)
    c = (torch.tensor(in_shape, dtype=torch.float64) - 1) / 2
    crop = torch.tensor([(s - o) // 2 for s, o in zip(in_shape, out_shape)], dtype=torch.float64)
    folded = c + m @ (crop - c) + torch.as_tensor(t, dtype=torch.float64)
    row = torch.zeros(16, dtype=torch.float64)
    row[:12] = torch.cat((m, folded[:, None]), 1).reshape(12)
    row[12], row[13] = gain, offset
    return row.to(torch.float32)


def table(tag, n=N, in_shape=IN_SHAPE, out_shape=None):
    """The table of a map: sample 0 as listed; every odd sample with the angles and t negated (another map of the same kind)."""
    from transoar_amd.augment import _rotation
    angles, divisor, signs, t, listed_out, gain, offset = MAPS[tag]
    out_shape = listed_out if out_shape is None else out_shape
    rows = []
    for i in range(n):
        sg = 1.0 if i % 2 == 0 else -1.0
        m = _rotation([sg * a for a in angles]) * torch.tensor(signs, dtype=torch.float64)[None, :] / divisor
        rows.append(raw_table(m, [sg * x for x in t], in_shape, out_shape, gain, offset))
    return torch.stack(rows), out_shape


@functools.lru_cache(maxsize=None)
def reference(tag):
    """-> (image fp32, labels int64, table, out_shape, fp64 image, labels, near-tie mask) of a map on the shared inputs."""
    from transoar_amd.augment import augment_torch
    image, labels = inputs()
    params, out_shape = table(tag)
    ref, ref_lab = augment_torch(image, labels, params, out_shape, A_MIN, A_MAX, dtype=torch.float64)
    return image, labels, params, out_shape, ref, ref_lab, near_tie(params, out_shape)


def near_tie(params, out_shape):
    """Voxels whose source coordinate lies within BAND of a half-integer on some axis (fp64 arithmetic on the fp32 table)."""
    p = params.to(torch.float64)
    n = p.shape[0]
    d, h, w = (torch.arange(s, dtype=torch.float64).view(v) for s, v in zip(out_shape, ((1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1))))
    band = torch.zeros(n, *out_shape, dtype=torch.bool)
    for a in range(3):
        m = p[:, 4 * a:4 * a + 4].view(n, 4, 1, 1, 1)
        s = m[:, 0] * d + m[:, 1] * h + m[:, 2] * w + m[:, 3]
        band |= ((s - s.floor()) - 0.5).abs() < BAND
    return band


def tensor_max_normalised(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def shipped_config(patch=None, median=IN_SHAPE):
    """The augmentation block of the reference's attn_fpn_foc_dec_{visceral,amos}.yaml (values only), on a toy volume."""
    aug = dict(use_augmentation=True, patch_size=None if patch is None else list(patch),
               p_gaussian_noise=0, p_gaussian_smooth=0, p_intensity_scale=0.5, p_intensity_shift=0.5, p_adjust_contrast=0,
               p_rotate=0.5, p_zoom=0.5, p_shear=0.0, p_translate=0.5, p_flip=0,
               gaussian_noise_mean=0.0, gaussian_noise_std=0.1, gaussian_smooth_sigma=[0.5, 1.0],
               intensity_scale_factors=0.1, intensity_shift_offsets=0.1, adjust_contrast_gamma=[0.7, 1.5],
               rotation=[-15, 15], min_zoom=0.8, max_zoom=1.2, translate_precentage=10, shear_range=[0.1, 0.1, 0.1],
               flip_axis=[0, 1, 2])
    return dict(augmentation=aug, foreground_voxel_statistics=dict(percentile_00_5=A_MIN, percentile_99_5=A_MAX),
                shape_statistics=dict(median=list(median)))
