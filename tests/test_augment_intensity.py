"""CPU: the opt-in steps of the batch augmentation (transoar_amd/augment.py, include/transoar_augment.h) -- Philox known answers,
the restatement of the intensity tail (intensity_torch) against independently written loops and closed formulas, shear in
compose_params against the steps' coordinate maps one after another, BatchAugment(full_chain=True)'s draws and refusals, and the
library's argument checks (no kernel is launched).

MONAI is not installed: the smoothing taps, the contrast formula and the order of the shear coefficients are MONAI's as the
header restates them, and the yardstick is that restatement."""
import ctypes
import math

import pytest
import torch

from tests._aug_inputs import IN_SHAPE, shipped_config
from tests._aug_intensity_inputs import CONTRAST, NOISE, SMOOTH, base, full_config


# ---- 1. Philox4x32-10 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    from transoar_amd.augment import philox4x32
    assert " ".join("%08x" % int(x) for x in philox4x32(counter, key)) == want
    # and as a batch: the words of a tensor of counters are those of each counter alone
    many = philox4x32([torch.tensor([c, 5]) for c in counter], key)
    assert " ".join("%08x" % int(x[0]) for x in many) == want


# ---- 2. the restatement ----------------------------------------------------------------------------------------------------------
def _taps(sigma):
    """MONAI's GaussianFilter(approx='erf', truncated=4) for an fp32 sigma, in plain Python."""
    sigma = float(torch.tensor(sigma, dtype=torch.float32))
    tail = int(max(4 * sigma, 0.5) + 0.5)
    t = 0.70710678 / sigma
    w = [max(0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5))), 0.0) for x in range(-tail, tail + 1)]
    return tail, [x / sum(w) for x in w]


@pytest.mark.parametrize("sigma,tail", [(0.1, 1), (0.125, 1), (0.5, 2), (0.625, 3), (1.0, 4), (4.0, 16)])
def test_smoothing_radius(sigma, tail):
    from transoar_amd.augment import smooth_tail, smooth_weights
    assert smooth_tail(sigma) == tail == _taps(sigma)[0]
    w = smooth_weights(sigma)
    assert w.numel() == 2 * tail + 1 and abs(float(w.sum()) - 1) <= 1e-14 and torch.equal(w, w.flip(0))
    assert float((w - torch.tensor(_taps(sigma)[1], dtype=torch.float64)).abs().max()) <= 1e-14


def test_smoothing_against_a_loop_over_taps():
    """<= 1e-12 in fp64 against three nested loops, on a volume smaller than the stencil in every axis, per-sample sigmas."""
    from transoar_amd.augment import compose_intensity, intensity_torch
    g = torch.Generator().manual_seed(3)
    image = torch.rand(2, 7, 5, 9, generator=g)
    sigmas = [[1.0, 0.5, 0.625], [0.3, 1.0, 0.8]]
    got = intensity_torch(image, compose_intensity(2, flags=SMOOTH, sigma=sigmas), dtype=torch.float64)
    for n in range(2):
        x = image[n].double()
        for axis in range(3):
            tail, w = _taps(sigmas[n][axis])
            x = x.movedim(axis, 0)
            y = torch.zeros_like(x)
            for i in range(x.shape[0]):
                for k, wk in zip(range(-tail, tail + 1), w):
                    if 0 <= i + k < x.shape[0]:
                        y[i] += wk * x[i + k]
            x = y.movedim(0, axis)
        err = float((got[n] - x).abs().max())
        print("sample %d: %.3g" % (n, err))
        assert err <= 1e-12, err


def test_constant_volume_and_its_faces():
    from transoar_amd.augment import compose_intensity, intensity_torch
    one = torch.ones(1, 24, 20, 36)
    got = intensity_torch(one, compose_intensity(1, flags=SMOOTH, sigma=[1.0, 1.0, 1.0]), dtype=torch.float64)[0]
    assert float((got[4:-4, 4:-4, 4:-4] - 1).abs().max()) <= 1e-12
    tail, w = _taps(1.0)
    inner = sum(w[tail:])                                    # the taps x >= 0: what a face keeps
    assert abs(float(got[0, 10, 18]) - inner) <= 1e-12 and abs(float(got[12, 19, 18]) - inner) <= 1e-12
    assert abs(float(got[12, 10, 0]) - inner) <= 1e-12 and abs(float(got[0, 0, 35]) - inner ** 3) <= 1e-12
    assert abs(float(got[1, 10, 18]) - sum(w[tail - 1:])) <= 1e-12


def test_contrast_against_the_closed_formula():
    from transoar_amd.augment import compose_intensity, intensity_torch
    image = base()
    table = compose_intensity(2, flags=[CONTRAST, CONTRAST], gamma=[0.7, 1.5], gain=1.05, offset=-0.1)
    got = intensity_torch(image, table, dtype=torch.float64)
    f = table.view(torch.float32).double()
    for n in range(2):
        x = image[n].double() * f[n, 6]
        x = x + f[n, 7]
        lo, hi = float(x.min()), float(x.max())
        want = ((x - lo) / (hi - lo + 1e-7)) ** float(f[n, 8]) * (hi - lo) + lo
        assert float((got[n] - want).abs().max()) <= 1e-12
        assert abs(float(got[n].min()) - lo) <= 1e-12 and abs(float(got[n].max()) - hi) <= 1e-6
    # skipped for a gamma that is not a finite positive number, and without the flag
    for gamma, flags in ((float("nan"), CONTRAST), (0.0, CONTRAST), (-1.0, CONTRAST), (float("inf"), CONTRAST), (0.7, 0)):
        same = intensity_torch(image, compose_intensity(2, flags=flags, gamma=gamma))
        assert torch.equal(same, image), gamma


def test_noise_statistics_and_keys():
    """Mean within 5 sigma / sqrt(n) and std within 5 sigma / sqrt(2 n) of the table's values over the 34 560 voxels of two
    samples; a voxel's noise depends on (key, index) only."""
    from transoar_amd.augment import compose_intensity, intensity_torch, philox_normals
    zero = torch.zeros(2, 24, 20, 36)
    mean, std = 0.02, 0.1
    table = compose_intensity(2, flags=NOISE, noise_mean=mean, noise_std=std, keys=[[1, 2], [1, 3]])
    got = intensity_torch(zero, table, dtype=torch.float64)
    n = got.numel()
    m, s = float(got.mean()), float(got.std())
    print("mean %.6f std %.6f over %d" % (m, s, n))
    assert n == 34560 and abs(m - _f32(mean)) <= 5 * std / math.sqrt(n) and abs(s - _f32(std)) <= 5 * std / math.sqrt(2 * n)
    assert not torch.equal(got[0], got[1])                   # another key
    again = intensity_torch(torch.ones(2, 24, 20, 36), table, dtype=torch.float64) - 1
    assert float((again - got).abs().max()) <= 1e-15          # other data, the same noise
    z = philox_normals(1000, [1], [2])
    assert torch.equal(z[0, :997], philox_normals(997, [1], [2])[0]) and abs(float(z.mean())) < 0.2
    want = (got[0].reshape(-1)[:1000] - _f32(mean)) / _f32(std)
    assert float((z[0] - want).abs().max()) <= 1e-12
    # a mean or std that is not finite skips the step
    for bad in (dict(noise_mean=float("nan")), dict(noise_std=float("inf"))):
        assert torch.equal(intensity_torch(zero, compose_intensity(2, flags=NOISE, **bad)), zero)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def test_invalid_sigma_skips_smoothing_for_that_row():
    from transoar_amd.augment import compose_intensity, intensity_torch
    image = base()
    good = intensity_torch(image, compose_intensity(2, flags=SMOOTH, sigma=[1.0, 1.0, 1.0]))
    for bad in (float("nan"), -1.0, 0.0, 1e9, 4.5):
        got = intensity_torch(image, compose_intensity(2, flags=SMOOTH, sigma=[[1.0, 1.0, 1.0], [1.0, bad, 1.0]]))
        assert torch.equal(got[0], good[0]) and torch.equal(got[1], image[1]), bad
    # the order is noise -> smooth -> gain -> offset -> contrast: gain and offset do not commute with the zero padding
    table = compose_intensity(2, flags=SMOOTH, sigma=[1.0, 1.0, 1.0], gain=1.1, offset=0.3)
    want = intensity_torch(image, compose_intensity(2, flags=SMOOTH, sigma=[1.0, 1.0, 1.0]), dtype=torch.float64) * _f32(1.1) + _f32(0.3)
    assert float((intensity_torch(image, table, dtype=torch.float64) - want).abs().max()) <= 1e-12
    five = intensity_torch(image[:, None], table)
    assert five.shape == (2, 1, 24, 20, 36) and torch.equal(five[:, 0], intensity_torch(image, table))


# ---- 3. shear ------------------------------------------------------------------------------------------------------------------
def test_shear_map_equals_the_steps_one_after_another():
    from transoar_amd.augment import _rotation, compose_params
    n = 3
    g = torch.Generator().manual_seed(9)
    rnd = lambda *shape: 2 * torch.rand(*shape, dtype=torch.float64, generator=g) - 1
    angles, zoom, translate = 20 * rnd(n, 3), 1 + 0.2 * rnd(n), 3 * rnd(n, 3)
    shear, flips = 0.1 * rnd(n, 6), torch.tensor([[1, 0, 0], [0, 1, 1], [0, 0, 0]], dtype=torch.bool)
    crop = torch.tensor([[3.0, 0.0, 5.0], [0.0, 2.0, 0.0], [1.0, 1.0, 2.0]], dtype=torch.float64)
    kw = dict(angles=angles, zoom=zoom, translate=translate, flips=flips, crop=crop)
    table = compose_params(n, IN_SHAPE, shear=shear, **kw)
    assert torch.equal(compose_params(n, IN_SHAPE, **kw), compose_params(n, IN_SHAPE, shear=None, **kw))
    plain = compose_params(n, IN_SHAPE, shear=torch.zeros(n, 6, dtype=torch.float64), **kw)
    assert float((plain - compose_params(n, IN_SHAPE, **kw)).abs().max()) <= 1e-5           # S = I is today's map (another rounding order)
    size = torch.tensor(IN_SHAPE, dtype=torch.float64)
    c = (size - 1) / 2
    o = torch.stack(torch.meshgrid(*[torch.arange(0.0, 4.0, dtype=torch.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for i in range(n):
        s01, s02, s10, s12, s20, s21 = shear[i].tolist()
        sh = torch.tensor([[1, s01, s02], [s10, 1, s12], [s20, s21, 1]], dtype=torch.float64)
        x = o + crop[i]                                                                    # crop: output -> flipped frame
        x = torch.where(flips[i], size - 1 - x, x)                                         # flip
        x = c + (x - c) @ sh.T                                                             # shear about the centre
        x = x - translate[i]                                                               # translate
        x = c + (x - c) / zoom[i]                                                          # zoom about the centre
        x = c + (x - c) @ _rotation(angles[i].tolist()).T                                  # rotate about the centre
        # the table is rounded to fp32 once: compare with the fp64 map the table was rounded from, at the rounding's size
        m = table[i, :12].double().view(3, 4)
        got = o @ m[:, :3].T + m[:, 3]
        assert float((got - x).abs().max()) <= 4 * 24 * 2.0 ** -24 * 40                    # fp32 entries of magnitude <= 40
        exact = _fp64_rows(i, angles, zoom, translate, flips, crop, sh, size, c)
        assert float((o @ exact[:, :3].T + exact[:, 3] - x).abs().max()) <= 1e-12
        assert torch.equal(exact.to(torch.float32), table[i, :12].view(3, 4))


def _fp64_rows(i, angles, zoom, translate, flips, crop, sh, size, c):
    """M = (R / z) S F and t = c + (R / z) (S (F k + f - c) - tr), in fp64, as the issue states them."""
    from transoar_amd.augment import _rotation
    a = _rotation(angles[i].tolist()) / zoom[i]
    sign = 1 - 2 * flips[i].double()
    m = (a @ sh) * sign[None, :]
    t = c + a @ (sh @ (sign * crop[i] + flips[i].double() * (size - 1) - c) - translate[i])
    return torch.cat((m, t[:, None]), 1)


# ---- 4. BatchAugment(full_chain=True) ------------------------------------------------------------------------------------------
def test_full_chain_with_probabilities_zero_is_the_default():
    from transoar_amd.augment import BatchAugment
    cfg = shipped_config(patch=(16, 12, 20))
    a, b = BatchAugment(cfg, "train", seed=11), BatchAugment(cfg, "train", seed=11, full_chain=True)
    assert b.tail_steps == 0
    for _ in range(3):
        table, tail = b.draw_both(8, IN_SHAPE)
        assert tail is None and torch.equal(table, a.draw(8, IN_SHAPE))
    image = base()
    x, _ = BatchAugment(cfg, "train", seed=4)(image)
    y, _ = BatchAugment(cfg, "train", seed=4, full_chain=True)(image)
    assert torch.equal(x, y)
    # 'val' and 'test' are unaffected, whatever the probabilities
    v = BatchAugment(full_config(1.0, patch=(16, 12, 20)), "val", seed=2, deterministic=True, full_chain=True)
    assert v.tail_steps == 0 and v.draw_both(2, IN_SHAPE)[1] is None
    assert torch.equal(v.draw(2, IN_SHAPE), BatchAugment(cfg, "val", seed=2, deterministic=True).draw(2, IN_SHAPE))


def test_full_chain_keeps_the_existing_draws():
    """The opt-in steps draw from a second generator: the spatial map is that of the default chain, gain and offset move from the
    resample's table into the tail's."""
    from transoar_amd.augment import BatchAugment
    cfg = full_config(1.0, patch=(16, 12, 20))
    cfg["augmentation"]["p_shear"] = 0.0
    plain = BatchAugment(shipped_config(patch=(16, 12, 20)), "train", seed=5).draw(16, IN_SHAPE)
    full = BatchAugment(cfg, "train", seed=5, full_chain=True)
    assert full.tail_steps == NOISE | SMOOTH | CONTRAST
    table, tail = full.draw_both(16, IN_SHAPE)
    assert torch.equal(table[:, :12], plain[:, :12]) and torch.equal(table[:, 12:], torch.tensor([1.0, 0, 0, 0]).expand(16, 4))
    assert tail.shape == (16, 12) and tail.dtype == torch.int32 and torch.equal(tail.view(torch.float32)[:, 6:8], plain[:, 12:14])
    assert int(tail[:, 11].abs().sum()) == 0
    # with shear the map differs, and only where the shear is
    cfg["augmentation"]["p_shear"] = 1.0
    sheared = BatchAugment(cfg, "train", seed=5, full_chain=True).draw(16, IN_SHAPE)
    assert not torch.equal(sheared[:, :12], plain[:, :12]) and float((sheared[:, :12] - plain[:, :12]).abs().max()) < 10


def test_full_chain_draws_respect_the_ranges():
    from transoar_amd.augment import BatchAugment
    aug = BatchAugment(full_config(1.0), "train", seed=3, full_chain=True)
    steps = aug.sample(500, IN_SHAPE)
    sh = steps["shear"]
    assert sh.shape == (500, 6) and float(sh[:, :3].abs().max()) <= 0.1 and float(sh[:, :3].abs().max()) > 0.09
    assert float(sh[:, 3:].abs().max()) == 0.0                       # shear_range has three entries: padded with zeros
    t = aug.sample_intensity(500)
    assert torch.equal(t["flags"], torch.full((500,), 7))
    assert float(t["noise_std"].min()) >= 0 and 0.09 < float(t["noise_std"].max()) <= 0.1
    assert float(t["sigma"].min()) >= 0.5 and float(t["sigma"].max()) <= 1.0 and t["sigma"].shape == (500, 3)
    assert float((t["sigma"][:, 0] - t["sigma"][:, 1]).abs().min()) > 0          # drawn independently per axis
    assert float(t["gamma"].min()) >= 0.7 and float(t["gamma"].max()) <= 1.5
    keys = t["keys"]
    assert int(keys.min()) >= 0 and int(keys.max()) < 2 ** 32 and int(keys.max()) >= 2 ** 31
    assert len(set(map(tuple, keys.tolist()))) == 500                # differ between samples
    assert not torch.equal(aug.sample_intensity(500)["keys"], keys)  # and between calls
    same = BatchAugment(full_config(1.0), "train", seed=3, full_chain=True)
    same.sample(500, IN_SHAPE)
    assert torch.equal(same.sample_intensity(500)["keys"], keys)     # seeded
    # pairs (a, b) draw U(a, b); half of the samples take a step at p = 0.5
    cfg = full_config(0.5)
    cfg["augmentation"]["shear_range"] = [[0.05, 0.1], 0.0, 0.0, 0.0, 0.0, [-0.2, -0.1]]
    half = BatchAugment(cfg, "train", seed=1, full_chain=True)
    sh = half.sample(2000, IN_SHAPE)["shear"]
    on = sh[:, 0] != 0
    assert 0.42 <= float(on.double().mean()) <= 0.58
    assert float(sh[on, 0].min()) >= 0.05 and float(sh[on, 0].max()) <= 0.1 and float(sh[on, 5].min()) >= -0.2 and float(sh[on, 5].max()) <= -0.1
    flags = half.sample_intensity(2000)["flags"]
    for bit in (NOISE, SMOOTH, CONTRAST):
        assert 0.42 <= float(((flags & bit) != 0).double().mean()) <= 0.58


@pytest.mark.parametrize("key,value", [("gaussian_smooth_sigma", [0.5, 4.5]), ("gaussian_smooth_sigma", [0.0, 1.0]),
                                       ("adjust_contrast_gamma", [0.0, 1.5]), ("adjust_contrast_gamma", [-0.5, 1.5]),
                                       ("gaussian_noise_std", -0.1), ("shear_range", [0.1] * 7)])
def test_full_chain_refusals_name_the_key(key, value):
    from transoar_amd.augment import BatchAugment
    cfg = full_config(1.0)
    cfg["augmentation"][key] = value
    with pytest.raises(ValueError, match=key):
        BatchAugment(cfg, "train", seed=0, full_chain=True)


@pytest.mark.parametrize("key", ["p_gaussian_noise", "p_gaussian_smooth", "p_adjust_contrast", "p_shear"])
def test_default_chain_points_to_full_chain(key):
    from transoar_amd.augment import BatchAugment
    cfg = shipped_config()
    cfg["augmentation"][key] = 0.2
    with pytest.raises(ValueError, match=key) as info:
        BatchAugment(cfg, "train", seed=0)
    assert "full_chain=True" in str(info.value)
    BatchAugment(cfg, "train", seed=0, full_chain=True)


def test_full_chain_on_cpu_tensors():
    """The CPU path of the whole chain: augment_torch then intensity_torch on the same draws, into out= when given."""
    from transoar_amd.augment import BatchAugment, augment_torch, intensity_torch
    from tests._aug_inputs import A_MAX, A_MIN, inputs
    image, labels = inputs()
    cfg = full_config(1.0, patch=(16, 12, 20))
    aug, twin = BatchAugment(cfg, "train", seed=8, full_chain=True), BatchAugment(cfg, "train", seed=8, full_chain=True)
    out = (torch.empty(2, 1, 16, 12, 20), torch.empty(2, 1, 16, 12, 20, dtype=torch.int64))
    x, lab = aug(image, labels, out=out)
    assert x is out[0] and lab is out[1]
    table, tail = twin.draw_both(2, IN_SHAPE)
    want, want_lab = augment_torch(image[:, None], labels[:, None], table, (16, 12, 20), A_MIN, A_MAX)
    assert torch.equal(x, intensity_torch(want, tail)) and torch.equal(lab, want_lab)
    assert not torch.equal(x, want)


# ---- 5. the library's argument checks ------------------------------------------------------------------------------------------
def test_intensity_argument_errors():
    from transoar_amd.augment import lib              # bound from include/transoar_augment.h
    f, size = lib.transoar_augment_intensity, lib.transoar_augment_intensity_workspace_bytes
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.transoar_augment_abi_version() == 1
    assert size(1) > 0 and size(3) == 3 * size(1) and size(1) % 4 == 0 and size(0) == 0 and size(-2) == 0
    ok = (2, 8, 8, 8)
    # NULL required pointers; scratch only with the smooth bit
    assert f(None, p, p, *ok, p, 7, p, None) == -1
    assert f(p, None, p, *ok, p, 7, p, None) == -1
    assert f(p, p, p, *ok, None, 7, p, None) == -1
    assert f(p, p, p, *ok, p, 7, None, None) == -1
    assert f(p, p, None, *ok, p, SMOOTH, p, None) == -1
    assert f(p, p, None, *ok, p, 7, p, None) == -1
    # extents below 1, too many samples, an extent above 2^24, a sample of 2^33 voxels
    for dims in ((0, 8, 8, 8), (2, 0, 8, 8), (2, 8, 0, 8), (2, 8, 8, -1), (65536, 8, 8, 8), (1, (1 << 24) + 1, 1, 1),
                 (1, 1 << 12, 1 << 12, 1 << 12)):
        assert f(p, p, p, *dims, p, 7, p, None) == -2, dims
        assert f(p, p, None, *dims, p, NOISE | CONTRAST, p, None) == -2, dims
    # misaligned pointers (a NULL scratch without the smooth bit is fine: the next thing wrong is reported)
    assert f(p + 2, p, p, *ok, p, 7, p, None) == -4
    assert f(p, p + 1, p, *ok, p, 7, p, None) == -4
    assert f(p, p, p + 3, *ok, p, 7, p, None) == -4
    assert f(p, p, p, *ok, p + 2, 7, p, None) == -4
    assert f(p, p, p, *ok, p, 7, p + 1, None) == -4
    assert f(p, p, None, *ok, p + 2, NOISE, p, None) == -4
