"""CPU: the batch augmentation (transoar_amd/augment.py, include/transoar_augment.h) -- the fp64 restatement against
torch.nn.functional.grid_sample, compose_params against the steps applied one after another, BatchAugment's draws, and the
library's argument checks (no kernel is launched).

MONAI is not installed, so there is no golden file from the reference for this feature: the yardstick is the fp64 restatement,
cross-checked here against grid_sample(align_corners=True, padding_mode='zeros')."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests._aug_inputs import A_MAX, A_MIN, DTYPES, IN_SHAPE, MAPS, N, reference, shipped_config, table, tensor_max_normalised


# ---- 1. the fp64 restatement against grid_sample -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(MAPS))
def test_restatement_against_grid_sample(tag):
    """Image <= 1e-10 tensor-max normalised (the project's fp64 bound), nearest labels equal.  Measured: at most 7e-15."""
    from transoar_amd.augment import _f32
    image, labels, params, out_shape, ref, ref_lab, _ = reference(tag)
    p = params.to(torch.float64)
    size = torch.tensor(IN_SHAPE, dtype=torch.float64)
    d, h, w = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in out_shape], indexing="ij")
    o = torch.stack((d, h, w, torch.ones_like(d)), -1)
    src = torch.einsum("nij,dhwj->ndhwi", p[:, :12].view(N, 3, 4), o)
    grid = (2 * src / (size - 1) - 1).flip(-1)                            # grid_sample wants (x, y, z) = (W, H, D)
    lo = torch.tensor(_f32(A_MIN), dtype=torch.float64)
    rng = (torch.tensor(_f32(A_MAX), dtype=torch.float32) - torch.tensor(_f32(A_MIN), dtype=torch.float32)).double()
    v = ((image.double() - lo) / rng).clamp(0, 1)
    want = F.grid_sample(v[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    want = want * p[:, 12].view(N, 1, 1, 1) + p[:, 13].view(N, 1, 1, 1)
    err = tensor_max_normalised(ref, want)
    print("%s: restatement against grid_sample %.3g" % (tag, err))
    assert err <= 1e-10, err
    want_lab = F.grid_sample(labels.double()[:, None], grid, mode="nearest", padding_mode="zeros", align_corners=True)[:, 0]
    # grid_sample rounds half to even and the restatement rounds half up: they can only differ at an exact tie, and the maps
    # with fractional coordinates have none (asserted), the exact map has integral coordinates
    assert torch.equal(want_lab.to(torch.int64), ref_lab)


def test_restatement_fp32_against_fp64():
    """The fp32 run of the restatement (the CPU path of augment) stays within the project's fp32 bound of its fp64 run, the labels
    differ only at near-ties; rank 5 and labels=None give the same image."""
    from transoar_amd.augment import augment, augment_torch
    for tag in sorted(MAPS):
        image, labels, params, out_shape, ref, ref_lab, band = reference(tag)
        got, got_lab = augment(image, labels, params, out_shape, A_MIN, A_MAX)
        assert got.dtype == torch.float32 and got_lab.dtype == labels.dtype and got.shape == (N, *out_shape)
        assert tensor_max_normalised(got, ref) <= 1e-4
        assert torch.equal(got_lab[~band], ref_lab[~band]) and float(band.float().mean()) <= 0.02
        five, five_lab = augment_torch(image[:, None], labels[:, None].to(torch.uint8), params, out_shape, A_MIN, A_MAX)
        assert five.shape == (N, 1, *out_shape) and torch.equal(five[:, 0], got)
        assert five_lab.dtype == torch.uint8 and torch.equal(five_lab[:, 0].long(), got_lab)
        alone, none = augment(image, None, params, out_shape, A_MIN, A_MAX)
        assert none is None and torch.equal(alone, got)


def test_coordinates_out_of_range_count_as_outside():
    from transoar_amd.augment import augment, augment_torch, check_table, compose_params
    image, labels, params, out_shape, _, _, _ = reference("exact")
    far = params.clone()
    far[:, 7] = 1e6                       # t of the H axis
    got, got_lab = augment(image, labels, far, out_shape, A_MIN, A_MAX)
    assert torch.equal(got, torch.zeros_like(got) + far[:, 13].view(N, 1, 1, 1)) and int(got_lab.abs().sum()) == 0
    for bad in (float("nan"), float("inf"), 3e7):
        broken = params.clone()
        broken[1, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            check_table(broken)
        with pytest.raises(ValueError, match="finite"):
            augment(image, labels, broken, out_shape, A_MIN, A_MAX)
        # the restatement itself treats such a coordinate as outside (what the kernel does with a device table)
        got, got_lab = augment_torch(image, labels, broken, out_shape, A_MIN, A_MAX)
        assert torch.equal(got[1], torch.zeros_like(got[1])) and int(got_lab[1].abs().sum()) == 0
        assert float(got[0].abs().sum()) > 0
    with pytest.raises(ValueError, match="zoom"):
        compose_params(1, IN_SHAPE, zoom=0.0)


# ---- 2. composition ------------------------------------------------------------------------------------------------------------
def test_composed_table_equals_the_steps_one_after_another():
    """A chain of 90-degree rotations, integer shifts, flips and a crop on a cube (so a rotation maps the frame onto itself and
    what a shift pushes out never comes back): one resample through compose_params' table is bit-identical to applying the steps
    one after another with the restatement.  a_min = 0, a_max = 1 on an image in [0, 1): the range scaling is the identity."""
    from transoar_amd.augment import augment_torch, compose_params
    side, out_shape, n = 12, (9, 12, 7), 3
    g = torch.Generator().manual_seed(5)
    image = torch.rand(n, side, side, side, generator=g)
    labels = torch.randint(0, 6, (n, side, side, side), generator=g)
    cube = (side,) * 3
    angles = torch.tensor([[90.0, 0.0, 0.0], [180.0, 270.0, 0.0], [-90.0, 90.0, 180.0]])
    shift = torch.tensor([[2.0, -3.0, 0.0], [0.0, 1.0, -4.0], [-1.0, 0.0, 5.0]])
    flips = torch.tensor([[1, 0, 0], [0, 1, 1], [1, 1, 1]], dtype=torch.bool)
    crop = torch.tensor([[3.0, 0.0, 5.0], [0.0, 0.0, 0.0], [1.0, 0.0, 2.0]])
    whole = compose_params(n, cube, angles=angles, translate=shift, flips=flips, crop=crop)
    m = whole[:, :12].view(n, 3, 4)
    assert bool(((m[:, :, :3] == 0) | (m[:, :, :3].abs() == 1)).all()) and torch.equal(m[:, :, 3], m[:, :, 3].round())
    assert int((m[:, :, :3] != 0).sum()) == 3 * n
    got, got_lab = augment_torch(image, labels, whole, out_shape, 0.0, 1.0)
    x, lab = image, labels
    for step in (dict(angles=angles), dict(translate=shift), dict(flips=flips)):
        x, lab = augment_torch(x, lab, compose_params(n, cube, **step), cube, 0.0, 1.0)
    x, lab = augment_torch(x, lab, compose_params(n, cube, crop=crop), out_shape, 0.0, 1.0)
    assert torch.equal(got.view(torch.int32), x.view(torch.int32)) and torch.equal(got_lab, lab)
    assert float((got != 0).float().mean()) > 0.3
    # and the single steps do what their names say
    flipped, _ = augment_torch(image, None, compose_params(n, cube, flips=[True, False, True]), cube, 0.0, 1.0)
    assert torch.equal(flipped, image.flip(1, 3))
    moved, _ = augment_torch(image, None, compose_params(n, cube, translate=[2.0, 0.0, -1.0]), cube, 0.0, 1.0)
    assert torch.equal(moved[:, 2:, :, :-1], image[:, :-2, :, 1:]) and float(moved[:, :2].abs().sum()) == 0
    window, _ = augment_torch(image, None, compose_params(n, cube, crop=[3, 0, 5]), out_shape, 0.0, 1.0)
    assert torch.equal(window, image[:, 3:12, :, 5:12])
    turned, _ = augment_torch(image, None, compose_params(n, cube, angles=[90.0, 0.0, 0.0]), cube, 0.0, 1.0)
    assert torch.equal(turned, image.rot90(1, (2, 3))) or torch.equal(turned, image.rot90(-1, (2, 3)))
    odd = image[:, :11, :11, :11].contiguous()           # centre 5: zoom 2 reads 5 + (o - 5) / 2, integral at the odd o
    bigger, _ = augment_torch(odd, None, compose_params(n, (11,) * 3, zoom=2.0), (11,) * 3, 0.0, 1.0)
    assert torch.equal(bigger[:, 1::2, 1::2, 1::2], odd[:, 3:8, 3:8, 3:8])


# ---- 3. BatchAugment's draws ---------------------------------------------------------------------------------------------------
def test_draws_are_seeded_and_respect_the_ranges():
    from transoar_amd.augment import BatchAugment
    cfg = shipped_config(patch=(16, 12, 20))
    a, b, c = BatchAugment(cfg, "train", seed=11), BatchAugment(cfg, "train", seed=11), BatchAugment(cfg, "train", seed=12)
    ta, tb, tc = a.draw(64, IN_SHAPE), b.draw(64, IN_SHAPE), c.draw(64, IN_SHAPE)
    assert ta.shape == (64, 16) and ta.dtype == torch.float32 and torch.equal(ta, tb) and not torch.equal(ta, tc)
    assert torch.equal(a.draw(64, IN_SHAPE), b.draw(64, IN_SHAPE)) and not torch.equal(a.draw(64, IN_SHAPE), ta)
    assert int(ta[:, 14:].abs().sum()) == 0
    steps = BatchAugment(cfg, "train", seed=3).sample(4000, IN_SHAPE)
    aug = cfg["augmentation"]
    assert float(steps["angles"].min()) >= -15 and float(steps["angles"].max()) <= 15
    assert float(steps["zoom"].min()) >= aug["min_zoom"] and float(steps["zoom"].max()) <= aug["max_zoom"]
    reach = torch.tensor(IN_SHAPE, dtype=torch.float64) * 0.1
    assert bool((steps["translate"].abs() <= reach).all())
    assert float((steps["gain"] - 1).abs().max()) <= 0.1 and float(steps["offset"].abs().max()) <= 0.1
    assert not bool(steps["flips"].any())                                  # p_flip = 0
    room = torch.tensor([8.0, 8.0, 16.0], dtype=torch.float64)
    assert bool((steps["crop"] >= 0).all()) and bool((steps["crop"] <= room).all()) and torch.equal(steps["crop"], steps["crop"].round())
    assert bool((steps["crop"] == room).any(0).all()) and bool((steps["crop"] == 0).any(0).all())      # both ends are reached
    # every step is applied to about half of the samples (p = 0.5; 4000 draws: +-8 % is more than five sigma)
    for name, applied in (("angles", (steps["angles"] != 0).any(1)), ("zoom", steps["zoom"] != 1), ("translate", (steps["translate"] != 0).any(1)),
                          ("gain", steps["gain"] != 1), ("offset", steps["offset"] != 0)):
        assert 0.42 <= float(applied.double().mean()) <= 0.58, name
    # a rotated sample uses the whole range on every axis
    assert float(steps["angles"].max(0).values.min()) > 14 and float(steps["angles"].min(0).values.max()) < -14


def test_all_probabilities_zero_is_the_identity():
    from transoar_amd.augment import BatchAugment, compose_params
    cfg = shipped_config()
    for key in ("p_rotate", "p_zoom", "p_translate", "p_flip", "p_intensity_scale", "p_intensity_shift"):
        cfg["augmentation"][key] = 0
    got = BatchAugment(cfg, "train", seed=1).draw(5)
    assert torch.equal(got, compose_params(5, IN_SHAPE))
    want = torch.zeros(16)
    want[0] = want[5] = want[10] = want[12] = 1
    assert torch.equal(got, want.expand(5, 16))
    # flips are drawn per axis when p_flip is on
    cfg["augmentation"]["p_flip"] = 1.0
    cfg["augmentation"]["flip_axis"] = [0, 2]
    assert torch.equal(BatchAugment(cfg, "train", seed=1).sample(3)["flips"], torch.tensor([[True, False, True]] * 3))


@pytest.mark.parametrize("key", ["p_gaussian_noise", "p_gaussian_smooth", "p_adjust_contrast", "p_shear"])
def test_unsupported_steps_raise(key):
    from transoar_amd.augment import BatchAugment
    cfg = shipped_config()
    cfg["augmentation"][key] = 0.2
    with pytest.raises(ValueError, match=key):
        BatchAugment(cfg, "train", seed=0)
    with pytest.raises(ValueError, match="split"):
        BatchAugment(shipped_config(), "training", seed=0)


@pytest.mark.parametrize("split", ["val", "test"])
def test_val_split_is_identity_plus_crop(split):
    from transoar_amd.augment import BatchAugment
    cfg = shipped_config(patch=(16, 12, 20))
    image, labels, _, _, _, _, _ = reference("exact")
    centred = BatchAugment(cfg, split, seed=0, deterministic=True)
    t = centred.draw(3, IN_SHAPE)
    want = torch.zeros(16)
    want[0] = want[5] = want[10] = want[12] = 1
    want[3], want[7], want[11] = 4, 4, 8
    assert torch.equal(t, want.expand(3, 16))
    x, lab = centred(image, labels.to(torch.int16))
    v = ((image - torch.tensor(A_MIN)) / (torch.tensor(A_MAX) - torch.tensor(A_MIN))).clamp(0, 1)
    assert x.shape == (N, 1, 16, 12, 20) and lab.shape == x.shape and lab.dtype == torch.int16
    assert torch.equal(x[:, 0], v[:, 4:20, 4:16, 8:28]) and torch.equal(lab[:, 0].long(), labels[:, 4:20, 4:16, 8:28])
    moving = BatchAugment(cfg, split, seed=0).draw(200, IN_SHAPE)
    assert torch.equal(moving[:, [0, 5, 10, 12]], torch.ones(200, 4)) and int(moving[:, [1, 2, 4, 6, 8, 9, 13, 14, 15]].abs().sum()) == 0
    assert len(set(map(tuple, moving[:, [3, 7, 11]].tolist()))) > 50
    assert bool((moving[:, [3, 7, 11]] <= torch.tensor([8.0, 8.0, 16.0])).all()) and bool((moving[:, [3, 7, 11]] >= 0).all())
    out = (torch.empty(N, 1, 16, 12, 20), torch.empty(N, 1, 16, 12, 20, dtype=torch.int16))
    x2, lab2 = centred(image, labels.to(torch.int16), out=out)
    assert x2 is out[0] and lab2 is out[1] and torch.equal(x2, x) and torch.equal(lab2, lab)
    with pytest.raises(ValueError, match="does not fit"):
        centred.draw(1, (10, 20, 36))


# ---- 4. the library's argument checks ------------------------------------------------------------------------------------------
def test_augment_argument_errors():
    from transoar_amd.augment import lib              # bound from include/transoar_augment.h
    f = lib.transoar_augment_forward
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    U8, I64 = 16, 19
    assert lib.transoar_augment_abi_version() == 1
    ok = (2, 8, 8, 8, 8, 8, 8)
    # NULL required pointers; labels and labels_out come together
    assert f(None, p, U8, *ok, p, 0.0, 1.0, p, p, None) == -1
    assert f(p, p, U8, *ok, None, 0.0, 1.0, p, p, None) == -1
    assert f(p, p, U8, *ok, p, 0.0, 1.0, None, p, None) == -1
    assert f(p, p, U8, *ok, p, 0.0, 1.0, p, None, None) == -1
    assert f(p, None, U8, *ok, p, 0.0, 1.0, p, p, None) == -1
    # bad dimensions: an extent below 1, an output above its input, too many samples, a sample of 2^40 voxels, an empty range
    for dims in ((0, 8, 8, 8, 8, 8, 8), (2, 0, 8, 8, 8, 8, 8), (2, 8, 8, 8, 0, 8, 8), (2, 8, 8, 8, 8, 8, -1), (2, 8, 8, 8, 9, 8, 8),
                 (2, 8, 8, 8, 8, 8, 9), (65536, 8, 8, 8, 8, 8, 8), (1, 1 << 14, 1 << 14, 1 << 12, 8, 8, 8),
                 (1, (1 << 24) + 1, 1, 1, 1, 1, 1)):
        assert f(p, p, U8, *dims, p, 0.0, 1.0, p, p, None) == -2, dims
    for lo, hi in ((1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (0.0, float("inf")), (-3e38, 3e38)):
        assert f(p, p, U8, *ok, p, lo, hi, p, p, None) == -2, (lo, hi)
    # unknown label dtype (not looked at without labels: dimensions are then the first thing wrong)
    assert f(p, p, 15, *ok, p, 0.0, 1.0, p, p, None) == -3
    assert f(p, p, 20, *ok, p, 0.0, 1.0, p, p, None) == -3
    # pointers not aligned to their element type
    assert f(p + 2, p, U8, *ok, p, 0.0, 1.0, p, p, None) == -4
    assert f(p, p, U8, *ok, p + 1, 0.0, 1.0, p, p, None) == -4
    assert f(p, p, U8, *ok, p, 0.0, 1.0, p + 3, p, None) == -4
    assert f(p, p + 4, I64, *ok, p, 0.0, 1.0, p, p, None) == -4
    assert f(p, p, I64, *ok, p, 0.0, 1.0, p, p + 4, None) == -4


def test_dtypes_of_the_tests_are_the_kernel_s():
    from transoar_amd import augment
    assert tuple(augment._LABEL_DT) == DTYPES and table("exact")[0].shape == (N, 16)
