"""The batch augmentation on its kernel (csrc/augment.hip, include/transoar_augment.h, transoar_amd/augment.py) against the fp64
restatement (augment_torch, cross-checked against grid_sample in tests/test_augment.py), computed once on the CPU and shared;
bit-identical against the fp32 restatement where the map is integer-exact; under a captured graph; and in front of the captured
training step, written straight into its static buffers.

Bounds: image <= 1e-4 tensor-max normalised (the project's fp32 bound, README "How parity is stated") and <= 1e-4 element-wise on
the entries above 1 % of the maximum; labels equal outside the near-tie band |frac(src) - 0.5| < 1e-3, which may hold at most 2 %
of the voxels (the maps' own shares are below 0.7 %)."""
import pytest
import torch

from tests._aug_inputs import A_MAX, A_MIN, DTYPES, IN_SHAPE, MAPS, N, inputs, near_tie, reference, shipped_config, table, tensor_max_normalised

pytestmark = pytest.mark.gpu
IDS = [str(d)[6:] for d in DTYPES]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _kernel(image, labels, params, out_shape, a_min=A_MIN, a_max=A_MAX, out=None):
    from transoar_amd import augment
    assert augment.usable(image, labels), "the kernel must take this input (no quiet torch path in a kernel test)"
    return augment.augment(image, labels, params, out_shape, a_min, a_max, out=out)


def _check_image(got, ref, what):
    got, ref = got.double().cpu(), ref.double()
    err = tensor_max_normalised(got, ref)
    big = ref.abs() > 0.01 * ref.abs().max()
    rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-30))[big].max())
    print("%s: tensor-max normalised %.3g, element-wise above 1 %% of the maximum %.3g" % (what, err, rel))
    assert err <= 1e-4, (what, err)
    assert rel <= 1e-4, (what, rel)


# ---- 1. the kernel against the fp64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["shipped", "zoomout", "crop"])
def test_kernel_against_fp64_restatement(tag):
    image, labels, params, out_shape, ref, ref_lab, band = reference(tag)
    share = float(band.double().mean())
    print("%s: near-tie share %.4f" % (tag, share))
    assert share <= 0.02
    for dtype in DTYPES:
        lab = labels.to(dtype).cuda()
        got, got_lab = _kernel(image.cuda(), lab, params, out_shape)
        assert got.shape == (N, *out_shape) and got.dtype == torch.float32 and got_lab.dtype == dtype
        _check_image(got, ref, "%s/%s" % (tag, dtype))
        got_lab = got_lab.cpu().long()
        assert torch.equal(got_lab[~band], ref_lab[~band])
        print("%s/%s: %d labels differ inside the band" % (tag, dtype, int((got_lab != ref_lab).sum())))
    alone, none = _kernel(image.cuda(), None, params, out_shape)
    assert none is None and torch.equal(alone, got)


# ---- 2. integer-exact maps: bit-identical to the fp32 restatement ---------------------------------------------------------------
def _exact_tables():
    """tag -> (table, out_shape): the issue's flip-and-shift map, the identity, and the validation split (identity + centred crop)."""
    from transoar_amd.augment import BatchAugment, compose_params
    val = BatchAugment(shipped_config(patch=(16, 12, 20)), "val", seed=0, deterministic=True)
    return {"exact": table("exact"), "identity": (compose_params(N, IN_SHAPE), IN_SHAPE), "val": (val.draw(N, IN_SHAPE), val.out_shape)}


@pytest.mark.parametrize("rank", [4, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_maps_are_bit_identical(dtype, rank):
    from transoar_amd.augment import augment_torch
    image, labels = inputs()
    labels = labels.to(dtype)
    if rank == 5:
        image, labels = image[:, None], labels[:, None]
    for tag, (params, out_shape) in _exact_tables().items():
        want, want_lab = augment_torch(image, labels, params, out_shape, A_MIN, A_MAX)          # fp32, on the CPU
        x, lab = image.cuda(), labels.cuda()
        kept_x, kept_lab = x.clone(), lab.clone()
        got, got_lab = _kernel(x, lab, params, out_shape)
        assert got.shape == want.shape and got_lab.shape == want_lab.shape and got_lab.dtype == dtype
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), tag
        assert torch.equal(got_lab.cpu(), want_lab), tag
        assert torch.equal(x, kept_x) and torch.equal(lab, kept_lab)
        alone, none = _kernel(x, None, params, out_shape)
        assert none is None and torch.equal(alone, got), tag
        assert float((want != 0).float().mean()) > 0.5 and int((want_lab != 0).sum()) > 0


def test_val_split_through_batch_augment():
    from transoar_amd.augment import BatchAugment
    image, labels = inputs()
    val = BatchAugment(shipped_config(patch=(16, 12, 20)), "val", seed=0, deterministic=True)
    want, want_lab = val(image, labels.to(torch.uint8))
    got, got_lab = val(image.cuda(), labels.to(torch.uint8).cuda())
    assert got.shape == (N, 1, 16, 12, 20) and got_lab.shape == got.shape
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(got_lab.cpu(), want_lab)
    # the ring of pinned slots wraps without corrupting a table: ten train draws, each equal to the CPU path of the same seed
    a, b = BatchAugment(shipped_config(), "train", seed=5), BatchAugment(shipped_config(), "train", seed=5)
    x, lab = image.cuda(), labels.to(torch.uint8).cuda()
    for _ in range(2 * BatchAugment.SLOTS + 2):
        got, got_lab = a(x, lab)
        want, want_lab = b(image, labels.to(torch.uint8))
        assert tensor_max_normalised(got.cpu(), want) <= 1e-4
        assert float((got_lab.cpu() != want_lab).float().mean()) <= 0.02


# ---- 3. coordinates outside, a table with a NaN --------------------------------------------------------------------------------
def test_far_translation_gives_offset_and_label_zero():
    image, labels, params, out_shape, _, _, _ = reference("shipped")
    for axis in range(3):
        far = params.clone()
        far[:, 4 * axis + 3] = 1e6
        got, got_lab = _kernel(image.cuda(), labels.to(torch.int16).cuda(), far, out_shape)
        assert torch.equal(got.cpu(), torch.zeros(N, *out_shape) + far[:, 13].view(N, 1, 1, 1)), axis
        assert int(got_lab.abs().sum()) == 0, axis


def test_nan_table_is_refused_on_the_host():
    image, labels, params, out_shape, _, _, _ = reference("shipped")
    out = (torch.full((N, *out_shape), 7.0, device="cuda"), torch.full((N, *out_shape), 7, dtype=torch.uint8, device="cuda"))
    for bad in (float("nan"), float("inf"), 1e8):
        broken = params.clone()
        broken[1, 6] = bad
        with pytest.raises(ValueError, match="finite"):
            _kernel(image.cuda(), labels.to(torch.uint8).cuda(), broken, out_shape, out=out)
    torch.cuda.synchronize()
    assert float(out[0].min()) == 7.0 == float(out[0].max()) and int(out[1].min()) == 7, "nothing was launched"


def test_device_table_out_of_range_counts_as_outside():
    """A device table is not read back; the kernel itself treats a coordinate that is not finite or beyond +-2^24 as outside
    (decided on the float: no address is formed from it)."""
    from transoar_amd.augment import augment_into
    image, labels, params, out_shape, _, _, _ = reference("exact")
    x, lab = image.cuda(), labels.to(torch.int32).cuda()
    for bad in (float("nan"), float("inf"), -float("inf"), 3e7, -3e38):
        broken = params.clone()
        broken[1, 11] = bad                    # t of the W axis, sample 1
        out = (torch.full((N, *out_shape), 7.0, device="cuda"), torch.full((N, *out_shape), 7, dtype=torch.int32, device="cuda"))
        augment_into(x, lab, broken.cuda(), out[0], out[1], A_MIN, A_MAX)
        good = _kernel(x, lab, params, out_shape)
        assert torch.equal(out[0][0], good[0][0]) and torch.equal(out[1][0], good[1][0])
        assert float(out[0][1].abs().max()) == 0.0 and int(out[1][1].abs().max()) == 0, bad


# ---- 4. odd sizes: scalar and vector stores, outputs written in full --------------------------------------------------------------
@pytest.mark.parametrize("shape,out_shape", [((1, 5, 6, 7), (5, 6, 7)), ((2, 13, 17, 70), (13, 17, 70)), ((2, 13, 17, 70), (11, 16, 66)),
                                             ((2, 13, 17, 70), (13, 17, 68)), ((3, 9, 10, 12), (7, 9, 8))],
                         ids=lambda s: "x".join(map(str, s)))
def test_odd_sizes_and_full_writes(shape, out_shape):
    """(1, 5, 6, 7) and (2, 13, 17, 70): samples that do not start on 16-byte boundaries and rows that are no multiple of four
    (scalar stores, masked tails); Wo = 68 and 8: the vector stores next to inputs whose rows are no multiple of four.  Outputs
    pre-filled with 0xFF bytes are written in full."""
    from transoar_amd.augment import augment_torch
    n, in_shape = shape[0], shape[1:]
    image, labels = inputs(in_shape, n, seed=sum(shape))
    for tag in ("shipped", "exact"):
        params, _ = table(tag, n, in_shape, out_shape)
        ref, ref_lab = augment_torch(image, labels, params, out_shape, A_MIN, A_MAX, dtype=torch.float64)
        band = near_tie(params, out_shape)
        for dtype in (torch.uint8, torch.int64):
            out = (torch.empty(n, *out_shape, device="cuda"), torch.empty(n, *out_shape, dtype=dtype, device="cuda"))
            out[0].view(torch.uint8).fill_(0xFF)              # a NaN in every float
            out[1].view(torch.uint8).fill_(0xFF)
            got, got_lab = _kernel(image.cuda(), labels.to(dtype).cuda(), params, out_shape, out=out)
            assert got is out[0] and got_lab is out[1]
            assert bool(torch.isfinite(got).all()) and int(got_lab.max()) <= 5 and int(got_lab.long().min()) >= 0
            _check_image(got, ref, "%s %s" % (tag, shape))
            got_lab = got_lab.cpu().long()
            assert torch.equal(got_lab[~band], ref_lab[~band]) and float(band.double().mean()) <= 0.02
            if tag == "exact":
                want, want_lab = augment_torch(image, labels, params, out_shape, A_MIN, A_MAX)
                assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(got_lab, want_lab)


def test_unaligned_output_views_take_the_scalar_stores():
    """Outputs that start 4 bytes (image) and 1 byte (labels) into an allocation: Wo is a multiple of four but a 16-byte store
    would be misaligned."""
    image, labels, params, out_shape, ref, ref_lab, band = reference("crop")
    count = N * out_shape[0] * out_shape[1] * out_shape[2]
    flat = (torch.zeros(count + 1, device="cuda"), torch.zeros(count + 1, dtype=torch.uint8, device="cuda"))
    out = (flat[0][1:].view(N, *out_shape), flat[1][1:].view(N, *out_shape))
    assert out[0].data_ptr() % 16 == 4
    got, got_lab = _kernel(image.cuda(), labels.to(torch.uint8).cuda(), params, out_shape, out=out)
    _check_image(got, ref, "unaligned")
    assert torch.equal(got_lab.cpu().long()[~band], ref_lab[~band])
    assert float(flat[0][0]) == 0.0 and int(flat[1][0]) == 0


# ---- 5. the bare op under a captured graph ---------------------------------------------------------------------------------------
def test_op_replays_in_a_graph():
    from transoar_amd.augment import augment_into
    image, labels, table_a, out_shape, _, _, _ = reference("shipped")
    table_b = reference("zoomout")[2]
    x, lab = image.cuda(), labels.to(torch.uint8).cuda()
    static = torch.zeros(N, 16, device="cuda")
    static[:, [0, 5, 10, 12]] = 1
    out = (torch.empty(N, *out_shape, device="cuda"), torch.empty(N, *out_shape, dtype=torch.uint8, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        augment_into(x, lab, static, out[0], out[1], A_MIN, A_MAX)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        augment_into(x, lab, static, out[0], out[1], A_MIN, A_MAX)
    for params in (table_a, table_b, table_a):
        static.copy_(params)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_lab = _kernel(x, lab, params, out_shape)
        assert torch.equal(out[0].view(torch.int32), eager.view(torch.int32)) and torch.equal(out[1], eager_lab)
    assert not torch.equal(_kernel(x, lab, table_a, out_shape)[0], _kernel(x, lab, table_b, out_shape)[0])


# ---- 6. in front of the captured training step -----------------------------------------------------------------------------------
def test_augment_writes_the_captured_step_s_inputs():
    """The configuration of tests/test_box_targets_gpu.py (lr = 0, one capture, targets=None): aug(raw, raw_labels,
    out=step.static_inputs()) followed by step(x, None, lab) replays on the augmented batch with no copy, and equals the eager
    step on aug's outputs within that file's 2e-3; two different draws separate the totals by more than 2e-2."""
    from tests.test_box_targets_gpu import _flagship_labels, _flagship_model
    from transoar_amd.augment import BatchAugment
    from transoar_amd.train_step import TrainStep, build_optimizer
    cfg, model, crit = _flagship_model(True)
    opt = build_optimizer(model, cfg)
    for group in opt.param_groups:
        group["lr"] = 0.0
    step = TrainStep(model, crit, cfg, optimizer=opt, amp_dtype=torch.bfloat16, graph=True)
    assert step.static_inputs() is None
    shape = tuple(cfg["volume_shape"])
    g = torch.Generator(device="cuda").manual_seed(1234)
    raw = torch.rand(2, 1, *shape, device="cuda", generator=g)
    raw_lab, _ = _flagship_labels(cfg)
    aug_cfg = shipped_config(patch=shape, median=shape)
    for key in ("p_rotate", "p_zoom", "p_translate", "p_intensity_scale", "p_intensity_shift"):
        aug_cfg["augmentation"][key] = 1.0                     # every draw moves the batch
    aug_cfg["augmentation"]["rotation"] = [-5, 5]
    aug_cfg["augmentation"]["min_zoom"], aug_cfg["augmentation"]["max_zoom"] = 0.9, 1.1
    aug = BatchAugment(aug_cfg, "train", seed=7)
    twin = BatchAugment(aug_cfg, "train", seed=7)              # the same draws, into fresh tensors, for the eager steps

    def eager(x, labels):
        side = step.capture_stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            total = float(step._eager_fwd_bwd(x, None, labels)[0])
        torch.cuda.current_stream().wait_stream(side)
        return total

    x1, lab1 = twin(raw, raw_lab)
    x2, lab2 = twin(raw, raw_lab)
    assert x1.shape == raw.shape and lab1.shape == raw_lab.shape and lab1.dtype == raw_lab.dtype
    e1, e2 = eager(x1, lab1), eager(x2, lab2)
    print("eager totals on two draws: %.6f %.6f" % (e1, e2))
    assert abs(e1 - e2) > 2e-2 * abs(e1), "the two draws must separate the totals: %r %r" % (e1, e2)
    step.capture(x1, None, lab1, warmup=1)
    static = step.static_inputs()
    assert static[0].shape == raw.shape and static[1].shape == raw_lab.shape
    totals = []
    for want_x, want_lab in ((x1, lab1), (x2, lab2)):
        x, lab = aug(raw, raw_lab, out=static)
        assert x.data_ptr() == static[0].data_ptr() and lab.data_ptr() == static[1].data_ptr()
        assert torch.equal(x, want_x) and torch.equal(lab, want_lab)
        totals.append(float(step(x, None, lab)[0]))
    print("replay totals: %.6f %.6f" % tuple(totals))
    assert abs(totals[0] - e1) <= 2e-3 * abs(e1), (totals[0], e1)
    assert abs(totals[1] - e2) <= 2e-3 * abs(e2), (totals[1], e2)
