"""Inputs of the intensity-tail tests (transoar_amd/augment.py: intensity_torch, intensity_into): the range-scaled base volume of
tests/_aug_inputs.py, the tables of the cases, and the fp64 restatement of each, computed once per process and never modified."""
import functools

import torch

from tests._aug_inputs import A_MAX, A_MIN, inputs, tensor_max_normalised

NOISE, SMOOTH, CONTRAST = 1, 2, 4

# tag -> the keywords of compose_intensity for the two samples.  'all': sample 0 has everything on, sample 1 noise and contrast
# only, with other sigmas (unused there), another gamma, gain and key.
CASES = {
    "noise": dict(flags=[NOISE, NOISE], noise_mean=[0.0, 0.02], noise_std=[0.05, 0.08], keys=[[11, 12], [13, 14]]),
    "smooth": dict(flags=[SMOOTH, SMOOTH], sigma=[[0.5, 1.0, 0.8], [1.0, 0.625, 0.55]]),
    "contrast": dict(flags=[CONTRAST, CONTRAST], gamma=[0.7, 1.5]),
    "all": dict(flags=[NOISE | SMOOTH | CONTRAST, NOISE | CONTRAST], noise_std=[0.05, 0.08], sigma=[[0.5, 1.0, 0.8], [1.0, 0.6, 0.7]],
                gain=[1.05, 0.95], offset=-0.1, gamma=[0.7, 1.5], keys=[[0xDEADBEEF, 7], [0xFFFFFFFF, 0x80000000]]),
    "gamma0.7": dict(flags=CONTRAST, gamma=0.7, offset=-0.1, gain=1.05),
    "gamma1.5": dict(flags=CONTRAST, gamma=1.5, offset=-0.1, gain=1.05),
}


@functools.lru_cache(maxsize=None)
def base(shape=None, n=2, seed=0):
    """The tests' volume after range scaling, (n, *shape) fp32 in [0, 1]."""
    image = inputs()[0] if shape is None else inputs(shape, n, seed)[0]
    lo, hi = torch.tensor(A_MIN, dtype=torch.float32), torch.tensor(A_MAX, dtype=torch.float32)
    return ((image - lo) / (hi - lo)).clamp(0, 1)


def steps_of(table):
    """The union of the rows' flags."""
    out = 0
    for f in table[:, 0].tolist():
        out |= f & 7
    return out


@functools.lru_cache(maxsize=None)
def reference(tag):
    """-> (image fp32, table, steps, fp64 restatement) of a case on the shared volume."""
    from transoar_amd.augment import compose_intensity, intensity_torch
    image = base()
    table = compose_intensity(image.shape[0], **CASES[tag])
    return image, table, steps_of(table), intensity_torch(image, table, dtype=torch.float64)


def errors(got, ref):
    """-> (tensor-max normalised, element-wise relative on the entries above 1 % of the maximum)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    big = ref.abs() > 0.01 * ref.abs().max()
    return tensor_max_normalised(got, ref), float(((got - ref).abs() / ref.abs().clamp_min(1e-30))[big].max())


def full_config(p=1.0, patch=None, median=None):
    """tests/_aug_inputs.shipped_config with the four opt-in probabilities at p."""
    from tests._aug_inputs import IN_SHAPE, shipped_config
    cfg = shipped_config(patch=patch, median=IN_SHAPE if median is None else median)
    for key in ("p_gaussian_noise", "p_gaussian_smooth", "p_adjust_contrast", "p_shear"):
        cfg["augmentation"][key] = p
    return cfg
