"""The case resize on its kernels (csrc/resize.hip, include/transoar_resize.h, transoar_amd/resize.py) against the fp64
restatement (resize_torch, cross-checked against F.interpolate in tests/test_resize.py), computed once on the CPU and shared;
bit-identical against the fp32 restatement where every sum is exact; the foreground window against its restatement and fed
straight into the resize from device memory; PrepareCase and TestSplit against their CPU paths; and under a captured graph.

Bounds: image <= 1e-4 tensor-max normalised (the project's fp32 bound, README "How parity is stated") and <= 1e-4 element-wise on
the entries above 1 % of the maximum; labels EQUAL (the nearest rule is integer-valued: no tie band, no share left out)."""
import pytest
import torch

from tests._resize_inputs import CASES, DTYPES, N, SHAPE, blobs, ct_inputs, inputs, reference, split_config, tensor_max_normalised, window_table

pytestmark = pytest.mark.gpu
IDS = [str(d)[6:] for d in DTYPES]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _kernel(image, labels, resized, out_shape=None, window=None, a_min=None, a_max=None, out=None):
    from transoar_amd import resize
    assert resize.usable(image, labels), "the kernel must take this input (no quiet torch path in a kernel test)"
    return resize.resize(image, labels, resized, out_shape, window=window, a_min=a_min, a_max=a_max, out=out)


def _window(labels, classes=None, margin=0):
    from transoar_amd import resize
    assert resize.usable(None, labels), "the kernels must take these labels (no quiet torch path in a kernel test)"
    return resize.foreground_window(labels, classes, margin)


def _check_image(got, ref, what):
    got, ref = got.double().cpu(), ref.double()
    err = tensor_max_normalised(got, ref)
    big = ref.abs() > 0.01 * ref.abs().max()
    rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-30))[big].max())
    print("%s: tensor-max normalised %.3g, element-wise above 1 %% of the maximum %.3g" % (what, err, rel))
    assert err <= 1e-4, (what, err)
    assert rel <= 1e-4, (what, rel)


# ---- 1. the kernel against the fp64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True], ids=["fp32", "int16"])
@pytest.mark.parametrize("scaled", [False, True], ids=["raw", "scaled"])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_kernel_against_fp64_restatement(tag, scaled, ct):
    image, labels, table, resized, out_shape, ref, ref_lab, lo, hi = reference(tag, scaled, ct)
    for dtype in DTYPES:
        got, got_lab = _kernel(image.cuda(), labels.to(dtype).cuda(), resized, out_shape, table, lo, hi)
        assert got.shape == (N, *out_shape) and got.dtype == torch.float32 and got_lab.dtype == dtype
        _check_image(got, ref, "%s/%s" % (tag, dtype))
        assert torch.equal(got_lab.cpu().long(), ref_lab), (tag, dtype)
    alone, none = _kernel(image.cuda(), None, resized, out_shape, table, lo, hi)
    assert none is None and torch.equal(alone, got)
    five, five_lab = _kernel(image[:, None].cuda(), labels[:, None].cuda(), resized, out_shape, table.cuda(), lo, hi)
    assert five.shape == (N, 1, *out_shape) and torch.equal(five[:, 0], got) and torch.equal(five_lab[:, 0].cpu(), ref_lab)


# ---- 2. exact sums: bit-identical to the fp32 restatement -----------------------------------------------------------------------
# (source shape, window rows or None, resized, out, crop): one-voxel bins (E == R, and E < R with R a multiple of E) and bins of 8
# on an integer-valued image; each with a crop and an out narrower than R, with an output width that is and is not a multiple of 4
ONE_VOXEL = [((12, 10, 18), None, (12, 10, 18), (12, 10, 18), (0, 0, 0)),
             ((12, 10, 18), None, (12, 10, 18), (9, 10, 16), (2, 0, 1)),
             ((12, 10, 18), None, (12, 10, 18), (12, 7, 13), (0, 3, 4)),
             ((12, 10, 18), ((1, 2, 3), (4, 5, 6)), (8, 15, 12), (8, 15, 12), (0, 0, 0)),
             ((12, 10, 18), ((1, 2, 3), (4, 5, 6)), (8, 15, 12), (7, 11, 9), (1, 3, 2)),
             ((12, 10, 18), ((1, 2, 3), (4, 5, 6)), (8, 15, 24), (5, 15, 20), (2, 0, 3))]
BINS_OF_8 = [((16, 24, 32), None, (8, 12, 16), (8, 12, 16), (0, 0, 0)),
             ((16, 24, 32), None, (8, 12, 16), (6, 12, 12), (1, 0, 3)),
             ((16, 24, 32), None, (8, 12, 16), (8, 9, 13), (0, 2, 1))]


def _exact_case(spec, integer, dtype, seed):
    from transoar_amd.resize import resize_torch
    shape, rows, resized, out, crop = spec
    image, labels = inputs(shape, N, seed)
    if integer:
        image = torch.randint(0, 256, (N, *shape), generator=torch.Generator().manual_seed(seed)).float()
    labels = labels.to(dtype)
    start, extent = ((0, 0, 0), shape) if rows is None else rows
    other = tuple(min(c + 1, r - o) for c, r, o in zip(crop, resized, out))             # the second sample: another crop
    table = window_table([(start, extent, crop), (start, extent, other)])
    want, want_lab = resize_torch(image, labels, table, resized, out)                    # fp32, on the CPU
    return image, labels, table, resized, out, want, want_lab


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,spec", [("one", s) for s in ONE_VOXEL] + [("eight", s) for s in BINS_OF_8],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[3])))
def test_exact_sums_are_bit_identical(family, spec, dtype):
    image, labels, table, resized, out, want, want_lab = _exact_case(spec, family == "eight", dtype, seed=sum(spec[3]))
    x, lab = image.cuda(), labels.cuda()
    kept_x, kept_lab = x.clone(), lab.clone()
    filled = (torch.empty(N, *out, device="cuda"), torch.empty(N, *out, dtype=dtype, device="cuda"))
    filled[0].view(torch.uint8).fill_(0xFF)              # a NaN in every float: the outputs are written in full
    filled[1].view(torch.uint8).fill_(0xFF)
    got, got_lab = _kernel(x, lab, resized, out, table, out=filled)
    assert got is filled[0] and got_lab is filled[1]
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(got_lab.cpu(), want_lab)
    assert torch.equal(x, kept_x) and torch.equal(lab, kept_lab)
    assert float((want != 0).float().mean()) > 0.5 and int((want_lab != 0).sum()) > 0
    if family == "eight":
        scaled = _kernel((x - 1000).to(torch.int16), lab, resized, out, table)[0]        # an int16 image: the same exact sums
        assert torch.equal(scaled.cpu(), want - 1000)


def test_unaligned_output_views_take_the_scalar_stores():
    """Outputs that start 4 bytes (image) and 1 byte (labels) into an allocation: Wo is a multiple of four but a 16-byte store
    would be misaligned."""
    image, labels, table, resized, out_shape, want, want_lab = _exact_case(BINS_OF_8[0], True, torch.uint8, seed=3)
    count = N * out_shape[0] * out_shape[1] * out_shape[2]
    flat = (torch.zeros(count + 1, device="cuda"), torch.zeros(count + 1, dtype=torch.uint8, device="cuda"))
    out = (flat[0][1:].view(N, *out_shape), flat[1][1:].view(N, *out_shape))
    assert out[0].data_ptr() % 16 == 4
    got, got_lab = _kernel(image.cuda(), labels.cuda(), resized, out_shape, table, out=out)
    assert torch.equal(got.cpu(), want) and torch.equal(got_lab.cpu(), want_lab)
    assert float(flat[0][0]) == 0.0 and int(flat[1][0]) == 0


def test_device_table_is_clamped_not_trusted():
    """A device table is not read back; the kernel clamps every row, so a broken row gives the result of its clamped row."""
    image, labels = inputs()
    resized, out = (22, 33, 22), (20, 33, 16)
    broken = window_table([((-5, 99, 4), (1000, 0, 52), (9, -2, 100)), ((1 << 30, 3, -(1 << 31)), (-(1 << 31), 39, (1 << 31) - 1), ((1 << 31) - 1, 0, 0))])
    clamped = window_table([((0, 42, 4), (30, 1, 52), (2, 0, 6)), ((29, 3, 0), (1, 39, 57), (2, 0, 0))])
    x, lab = image.cuda(), labels.cuda()
    want, want_lab = _kernel(x, lab, resized, out, clamped)
    got, got_lab = _kernel(x, lab, resized, out, broken.cuda())
    assert torch.equal(got, want) and torch.equal(got_lab, want_lab)
    with pytest.raises(ValueError, match="window"):
        _kernel(x, lab, resized, out, broken)                      # from the host it is refused


# ---- 3. the foreground window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_foreground_window_on_the_kernel(dtype):
    from transoar_amd.resize import foreground_window_torch
    lab = blobs(n=3, empty=1)
    lab[2, 0, 0, 0], lab[2, SHAPE[0] - 1, SHAPE[1] - 1, SHAPE[2] - 1] = 3, 3
    if dtype != torch.uint8:
        lab[0, 1, 1, 1], lab[0, 2, 2, 2] = -3, 300                 # neither is a class, nor "label > 0" for the negative one
    dev = lab.to(dtype).cuda()
    for classes, margin in ((None, 0), (None, (1, 30, 4)), ((1,), 2), ((3, 14), (100, 100, 100)), ((1, 6, 7, 14, 15), 2), ((2, 62), 1), ((40,), 0)):
        want = foreground_window_torch(lab.to(dtype), classes, margin)
        got = _window(dev, classes, margin)
        assert got.is_cuda and got.dtype == torch.int32 and torch.equal(got.cpu(), want), (classes, margin)
        assert int(want[1, 9]) == 0
    assert torch.equal(_window(dev[:, None], None, 2).cpu(), foreground_window_torch(lab.to(dtype), None, 2))


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 17, 33, 129), (3, 40, 64, 70)], ids=lambda s: "x".join(map(str, s)))
def test_foreground_window_sizes(shape):
    """One workgroup with scalar ends only; samples that do not start on a 16-byte boundary; several workgroups per sample
    (above 4096 voxels each), rows and planes crossed inside a 16-byte group."""
    from transoar_amd.resize import foreground_window_torch
    n, vol = shape[0], shape[1:]
    g = torch.Generator().manual_seed(sum(shape))
    for dtype in (torch.uint8, torch.int32):
        lab = torch.zeros(n, *vol, dtype=torch.int64)
        for s in range(n):
            at = [torch.randint(0, v, (4,), generator=g) for v in vol]
            lab[s, at[0], at[1], at[2]] = torch.tensor([1, 2, 5, 9])
        want = foreground_window_torch(lab.to(dtype), (1, 2, 5), 1)
        assert torch.equal(_window(lab.to(dtype).cuda(), (1, 2, 5), 1).cpu(), want)


def test_window_feeds_the_resize_from_device_memory():
    image, _ = inputs()
    lab = blobs().to(torch.uint8)
    x, dev = image.cuda(), lab.cuda()
    window = _window(dev, (1, 6, 7, 14, 15), 2)
    assert window.is_cuda
    got, got_lab = _kernel(x, dev, (12, 14, 16), window=window)
    want, want_lab = _kernel(x, dev, (12, 14, 16), window=window.cpu())           # the same table, checked and uploaded
    assert torch.equal(got, want) and torch.equal(got_lab, want_lab)
    assert not torch.equal(got, _kernel(x, dev, (12, 14, 16))[0])


# ---- 4. PrepareCase and TestSplit against their CPU paths ---------------------------------------------------------------------------
def test_prepare_case_against_its_cpu_path():
    from transoar_amd.resize import PrepareCase
    image, _ = ct_inputs()
    lab = blobs().to(torch.uint8)
    for prep in (PrepareCase((12, 14, 16), (1, 6, 7, 14, 15), 2), PrepareCase((33, 20, 64), None, 5)):
        want, want_lab, want_window = prep(image, lab)
        from transoar_amd import resize
        assert resize.usable(image.cuda(), lab.cuda())
        got, got_lab, window = prep(image.cuda(), lab.cuda())
        assert got.is_cuda and got.dtype == torch.float32 and got_lab.dtype == torch.int32 and window.is_cuda
        assert got.shape == (N, *prep.resize_shape) == got_lab.shape
        assert torch.equal(window.cpu(), want_window) and torch.equal(got_lab.cpu(), want_lab)
        _check_image(got, want, "PrepareCase %s" % (prep.resize_shape,))


def test_test_split_against_its_cpu_path():
    from transoar_amd import resize
    image, labels = inputs()
    labels = labels.to(torch.uint8)
    x, lab = image.cuda(), labels.cuda()
    assert resize.usable(x, lab)
    cfg = split_config((22, 33, 40), (16, 20, 32))
    a, b = resize.TestSplit(cfg, seed=5), resize.TestSplit(cfg, seed=5)
    out = (torch.empty(N, 1, 16, 20, 32, device="cuda"), torch.empty(N, 1, 16, 20, 32, dtype=torch.uint8, device="cuda"))
    seen = set()
    for i in range(10):                                             # the ring of pinned slots wraps (SLOTS = 4)
        want, want_lab = b.split(image, labels)
        got, got_lab = a.split(x, lab, out=out if i % 2 else None)
        if i % 2:
            assert got is out[0] and got_lab is out[1]
        assert got.shape == (N, 1, 16, 20, 32) and got_lab.shape == got.shape
        _check_image(got, want, "TestSplit draw %d" % i)
        assert torch.equal(got_lab.cpu(), want_lab)
        seen.add(float(want.double().sum()))
    assert len(seen) > 5 and resize.TestSplit.SLOTS < 10
    centred = resize.TestSplit(split_config((22, 33, 40)), deterministic=True)
    got, got_lab = centred(x, lab)
    want, want_lab = centred(image, labels)
    assert got.shape == (N, 1, 22, 33, 40)
    _check_image(got, want, "TestSplit whole")
    assert torch.equal(got_lab.cpu(), want_lab)


# ---- 5. one captured graph: foreground window, then resize ---------------------------------------------------------------------------
def test_window_then_resize_replays_in_a_graph():
    from transoar_amd import resize
    image_a, _ = ct_inputs()
    image_b, _ = ct_inputs(seed=9)
    lab_a = blobs().to(torch.uint8)
    lab_b = torch.roll(blobs(), (3, -2, 5), (1, 2, 3)).to(torch.uint8)
    resized, classes = (12, 14, 16), (1, 6, 7, 14, 15)
    x, lab = image_a.cuda(), lab_a.cuda()
    assert resize.usable(x, lab)
    window = torch.zeros(N, 12, dtype=torch.int32, device="cuda")
    ws = torch.empty(resize.workspace_bytes(N, lab[0].numel()) // 4, dtype=torch.int32, device="cuda")
    out = (torch.empty(N, *resized, device="cuda"), torch.empty(N, *resized, dtype=torch.uint8, device="cuda"))

    def run():
        resize.foreground_window_into(lab, window, ws, classes, 2)
        resize.resize_into(x, lab, window, resized, out[0], out[1], -200.0, 300.0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    eager = {}
    for tag, (im, lb) in (("a", (image_a, lab_a)), ("b", (image_b, lab_b))):
        w = _window(lb.cuda(), classes, 2)
        eager[tag] = (w,) + _kernel(im.cuda(), lb.cuda(), resized, window=w, a_min=-200.0, a_max=300.0)
    assert not torch.equal(eager["a"][0], eager["b"][0]) and not torch.equal(eager["a"][1], eager["b"][1])
    for tag, (im, lb) in (("b", (image_b, lab_b)), ("a", (image_a, lab_a)), ("b", (image_b, lab_b))):
        x.copy_(im)
        lab.copy_(lb)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(window, eager[tag][0]), tag
        assert torch.equal(out[0].view(torch.int32), eager[tag][1].view(torch.int32)) and torch.equal(out[1], eager[tag][2]), tag
