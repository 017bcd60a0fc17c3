"""The intensity tail on its kernels (csrc/augment.hip: transoar_augment_intensity) against the fp64 restatement (intensity_torch,
checked on the CPU in tests/test_augment_intensity.py), computed once on the CPU and shared; bit-identical where no step runs;
across every tile edge; under a captured graph; and behind the resample in BatchAugment(full_chain=True).

Bounds: <= 1e-4 tensor-max normalised (the project's fp32 bound) and <= 1e-4 element-wise on the entries above 1 % of the
maximum.  The fp32 run of the restatement itself stays below 5e-7 and 1e-6 of its fp64 run on these cases."""
import pytest
import torch

from tests._aug_inputs import A_MAX, A_MIN, IN_SHAPE, inputs, near_tie
from tests._aug_intensity_inputs import CASES, CONTRAST, NOISE, SMOOTH, base, errors, full_config, reference

pytestmark = pytest.mark.gpu
ALL = NOISE | SMOOTH | CONTRAST


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _kernel(image, table, steps, out=None):
    """The kernel sequence on a CPU or CUDA image and a host table -> the result on the device."""
    from transoar_amd import augment
    x = image.cuda()
    assert augment.usable(x), "the kernel must take this input (no quiet torch path in a kernel test)"
    out = torch.empty_like(x) if out is None else out
    return augment.intensity_into(x, out, table.cuda(), steps)


def _check(got, ref, what):
    err, rel = errors(got, ref)
    print("%s: tensor-max normalised %.3g, element-wise above 1 %% of the maximum %.3g" % (what, err, rel))
    assert err <= 1e-4, (what, err)
    assert rel <= 1e-4, (what, rel)


# ---- 6. each step alone and all together -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(CASES))
def test_kernel_against_fp64_restatement(tag):
    image, table, steps, ref = reference(tag)
    got = _kernel(image, table, steps)
    assert got.shape == image.shape and got.dtype == torch.float32
    _check(got, ref, tag)
    assert float((ref - image.double()).abs().max()) > 1e-2                   # the case does something
    # the passes of steps the rows do not use change nothing beyond the rounding of another path
    _check(_kernel(image, table, ALL), ref, tag + " with every pass launched")
    five = _kernel(image[:, None], table, steps)
    assert five.shape == (2, 1, *IN_SHAPE) and torch.equal(five[:, 0], got)


# ---- 7. nothing on: bit-identical ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [0, NOISE, NOISE | CONTRAST, SMOOTH, ALL])
def test_flags_off_is_bit_identical(steps):
    from transoar_amd.augment import compose_intensity
    image = base().clone()
    image[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 1e-40, -1e-40])            # signed zeros and denormals pass unchanged
    table = compose_intensity(2, flags=0, noise_std=0.3, sigma=[1.0, 1.0, 1.0], gamma=0.7, keys=[5, 6])
    got = _kernel(image, table, steps)
    assert torch.equal(got.cpu().view(torch.int32), image.view(torch.int32))
    # one sample on, the other off: the one that is off is bit-identical next to it
    if steps:
        table = compose_intensity(2, flags=[steps, 0], noise_std=0.3, sigma=[1.0, 1.0, 1.0], gamma=0.7, keys=[5, 6])
        got = _kernel(image, table, steps)
        assert torch.equal(got[1].cpu().view(torch.int32), image[1].view(torch.int32)) and not torch.equal(got[0].cpu(), image[0])


# ---- 8. shapes that cross every tile edge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sigma,in_place", [((2, 7, 5, 9), 1.0, False), ((1, 3, 33, 70), 1.0, False), ((1, 3, 33, 70), 1.0, True),
                                                  ((1, 20, 18, 40), 4.0, False), ((2, 5, 34, 68), 0.5, True), ((1, 2, 40, 132), 2.2, False)],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_tile_edges_and_full_writes(shape, sigma, in_place):
    """(2, 7, 5, 9): a radius of 4 exceeds half of every extent, samples do not start on 16-byte boundaries; (1, 3, 33, 70): W no
    multiple of 4 and one more row / six more columns than a 32 x 64 tile; (1, 20, 18, 40) with sigma 4: radius 16;
    (2, 5, 34, 68) and (1, 2, 40, 132): the 16-byte path across tile edges, radii 2 and 9 (R = 12).  Outputs pre-filled with 0xFF
    bytes are written in full."""
    from transoar_amd.augment import compose_intensity, intensity_torch
    n = shape[0]
    image = base(shape[1:], n, sum(shape))
    table = compose_intensity(n, flags=ALL, noise_std=0.05, sigma=[sigma, sigma, sigma], gain=1.05, offset=-0.1, gamma=0.7,
                              keys=[shape[1], shape[3]])
    ref = intensity_torch(image, table, dtype=torch.float64)
    x = image.cuda()
    kept = x.clone()
    if in_place:
        out = x
    else:
        out = torch.empty_like(x)
        out.view(torch.uint8).fill_(0xFF)                     # a NaN in every float
    got = _kernel(x, table, ALL, out=out)
    assert got.data_ptr() == out.data_ptr() and bool(torch.isfinite(got).all())
    _check(got, ref, "%s sigma %g" % (shape, sigma))
    if not in_place:
        assert torch.equal(x, kept)
        # smoothing alone through the same tiles (no contrast pass that could hide a border)
        alone = compose_intensity(n, flags=SMOOTH, sigma=[sigma, sigma, sigma])
        _check(_kernel(x, alone, SMOOTH), intensity_torch(image, alone, dtype=torch.float64), "%s smooth only" % (shape,))


def test_unaligned_views_take_the_scalar_path():
    """An image and an output that start 4 bytes into their allocations: W is a multiple of four but 16-byte accesses would be
    misaligned; the float in front of the output stays as it was."""
    image, table, steps, ref = reference("all")
    count = image.numel()
    src, dst = torch.zeros(count + 1, device="cuda"), torch.zeros(count + 1, device="cuda")
    src[1:].copy_(image.reshape(-1))
    x, out = src[1:].view(image.shape), dst[1:].view(image.shape)
    assert x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    _check(_kernel(x, table, steps, out=out), ref, "unaligned")
    assert float(dst[0]) == 0.0


# ---- 9. noise ------------------------------------------------------------------------------------------------------------------
def test_noise_is_keyed_and_equals_the_restatement_element_by_element():
    """On a zero image with mean 0 and std 1 the output IS the normal deviate of every voxel.  Against the fp64 restatement:
    |z| <= 5.8 (u1 >= 2^-24) and logf, sqrtf, sincospif carry a few ulp each, so 1e-5 absolute is more than ten times the fp32
    error.  Through the smooth-capable path (sigma off for the row, tiles with halos) the values are the same bits as through
    the element-wise path: a voxel's noise does not depend on the tiling."""
    from transoar_amd.augment import compose_intensity, philox_normals
    for shape in ((2, 24, 20, 36), (1, 3, 33, 70)):
        zero = torch.zeros(shape)
        keys = [[7, 8], [7, 9]][:shape[0]]
        table = compose_intensity(shape[0], flags=NOISE, noise_std=1.0, keys=keys)
        got = _kernel(zero, table, NOISE)
        want = philox_normals(zero[0].numel(), [k[0] for k in keys], [k[1] for k in keys]).view(shape)
        err = float((got.cpu().double() - want).abs().max())
        print("%s: noise against the restatement %.3g, largest |z| %.3f" % (shape, err, float(want.abs().max())))
        assert err <= 1e-5, err
        assert torch.equal(_kernel(zero, table, NOISE), got)                                 # the same key: the same bits
        assert torch.equal(_kernel(zero, table, NOISE | SMOOTH), got)                        # tiled with halos: the same bits
        if shape[0] == 2:
            assert not torch.equal(got[0], got[1])                                           # another key
    # the same key on other data: the same noise, another result
    image = base()
    table = compose_intensity(2, flags=NOISE, noise_std=0.1, keys=[3, 4])
    got = _kernel(image, table, NOISE)
    assert not torch.equal(got[0], got[1])
    z = philox_normals(image[0].numel(), [3], [4]).view(image[0].shape)
    assert float((got[0].cpu().double() - (image[0].double() + float(torch.tensor(0.1)) * z)).abs().max()) <= 2e-6
    # noise, then smoothing of the noisy volume: halo voxels carry their own tile's noise
    both = compose_intensity(2, flags=NOISE | SMOOTH, noise_std=0.1, sigma=[1.0, 1.0, 1.0], keys=[3, 4])
    from transoar_amd.augment import intensity_torch
    _check(_kernel(image, both, NOISE | SMOOTH), intensity_torch(image, both, dtype=torch.float64), "noise + smooth")


# ---- 10. what a device table may hold --------------------------------------------------------------------------------------------
def test_device_table_validation():
    from transoar_amd.augment import compose_intensity, intensity_torch
    image = base()
    common = dict(noise_std=0.05, gain=1.05, offset=-0.1, keys=[[1, 2], [3, 4]])
    for bad in (float("nan"), -1.0, 1e9, 0.0, float("inf")):
        table = compose_intensity(2, flags=ALL, sigma=[[1.0, 1.0, 1.0], [1.0, 1.0, bad]], gamma=0.7, **common)
        ref = intensity_torch(image, table, dtype=torch.float64)
        skipped = intensity_torch(image, compose_intensity(2, flags=[ALL, NOISE | CONTRAST], sigma=[1.0, 1.0, 1.0], gamma=0.7, **common),
                                  dtype=torch.float64)
        assert torch.equal(ref, skipped)                      # the restatement skips smoothing for that row only
        _check(_kernel(image, table, ALL), ref, "sigma %r" % bad)
    for bad in (float("nan"), 0.0, -0.7, float("inf")):
        table = compose_intensity(2, flags=ALL, sigma=[1.0, 0.5, 0.8], gamma=[bad, 1.5], **common)
        ref = intensity_torch(image, table, dtype=torch.float64)
        skipped = intensity_torch(image, compose_intensity(2, flags=[NOISE | SMOOTH, ALL], sigma=[1.0, 0.5, 0.8], gamma=[1.0, 1.5], **common),
                                  dtype=torch.float64)
        assert torch.equal(ref, skipped)
        _check(_kernel(image, table, ALL), ref, "gamma %r" % bad)
    # every flag bit set, steps = noise only: noise only (gain and offset always apply)
    table = compose_intensity(2, flags=0xFFFFFFFF, sigma=[float("nan"), 1e9, -1.0], gamma=float("nan"), **common)
    ref = intensity_torch(image, compose_intensity(2, flags=NOISE, **common), dtype=torch.float64)
    _check(_kernel(image, table, NOISE), ref, "flags 0xFFFFFFFF, steps NOISE")
    table = compose_intensity(2, flags=0xFFFFFFFF, sigma=[1.0, 1.0, 1.0], gamma=0.7, **common)
    _check(_kernel(image, table, NOISE), ref, "valid rows, steps NOISE")
    # a noise mean or std, gain or offset that is not finite skips its step
    table = compose_intensity(2, flags=ALL, noise_mean=[0.0, float("nan")], noise_std=[float("inf"), 0.05], sigma=[1.0, 1.0, 1.0],
                              gain=[float("nan"), 1.05], offset=[-0.1, float("inf")], gamma=0.7, keys=[1, 2])
    _check(_kernel(image, table, ALL), intensity_torch(image, table, dtype=torch.float64), "non-finite scalars")


# ---- 11. the bare op under a captured graph --------------------------------------------------------------------------------------
def test_op_replays_in_a_graph_with_fresh_keys():
    from transoar_amd.augment import compose_intensity, intensity_into, intensity_workspace
    image = base().cuda()
    kw = dict(flags=ALL, noise_std=0.05, sigma=[0.5, 1.0, 0.8], gain=1.05, offset=-0.1, gamma=1.5)
    tables = [compose_intensity(2, keys=keys, **kw) for keys in ([[1, 2], [3, 4]], [[5, 6], [7, 8]])]
    static = tables[0].cuda()
    out, scratch, workspace = torch.empty_like(image), torch.empty_like(image), intensity_workspace(2, image.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        intensity_into(image, out, static, ALL, scratch, workspace)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        intensity_into(image, out, static, ALL, scratch, workspace)
    seen = []
    for table in (tables[0], tables[1], tables[0]):
        static.copy_(table)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, _kernel(image, table, ALL))
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])


# ---- 12. behind the resample -----------------------------------------------------------------------------------------------------
def test_batch_augment_full_chain():
    from transoar_amd.augment import BatchAugment, augment_torch, intensity_torch
    image, labels = inputs()
    cfg = full_config(1.0, patch=(16, 12, 20))
    for key in ("p_rotate", "p_zoom", "p_translate", "p_intensity_scale", "p_intensity_shift"):
        cfg["augmentation"][key] = 1.0
    aug, twin = BatchAugment(cfg, "train", seed=21, full_chain=True), BatchAugment(cfg, "train", seed=21, full_chain=True)
    assert aug.tail_steps == ALL
    x, lab = image.cuda(), labels.to(torch.uint8).cuda()
    out = (torch.empty(2, 1, 16, 12, 20, device="cuda"), torch.empty(2, 1, 16, 12, 20, dtype=torch.uint8, device="cuda"))
    out[0].view(torch.uint8).fill_(0xFF)
    seen = []
    for _ in range(BatchAugment.SLOTS + 2):                   # the tail's ring wraps too
        got, got_lab = aug(x, lab, out=out)
        assert got.data_ptr() == out[0].data_ptr() and got_lab.data_ptr() == out[1].data_ptr()
        table, tail = twin.draw_both(2, IN_SHAPE)
        assert float(table[:, 12].min()) == 1.0 == float(table[:, 12].max()) and float(table[:, 13].abs().max()) == 0.0
        ref, ref_lab = augment_torch(image[:, None], labels[:, None], table, (16, 12, 20), A_MIN, A_MAX, dtype=torch.float64)
        _check(got, intensity_torch(ref, tail, dtype=torch.float64), "full chain")
        band = near_tie(table, (16, 12, 20))[:, None]
        assert float(band.double().mean()) <= 0.02
        assert torch.equal(got_lab.cpu().long()[~band], ref_lab[~band])
        seen.append(got.clone())
    assert not torch.equal(seen[0], seen[1])
    # nothing switched on: no tail, the default chain's output bit for bit
    plain_cfg = full_config(0.0, patch=(16, 12, 20))
    a, b = BatchAugment(plain_cfg, "train", seed=2, full_chain=True), BatchAugment(plain_cfg, "train", seed=2)
    assert a.tail_steps == 0 and torch.equal(a(x, lab)[0], b(x, lab)[0]) and not a._buffers
