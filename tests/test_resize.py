"""CPU: the case resize (transoar_amd/resize.py, include/transoar_resize.h) -- the torch restatement against
torch.nn.functional.interpolate (mode='area' in fp64 within 1e-12, mode='nearest' equal) on the sliced windows and on every pair
E, R in 1..48; the foreground window against a direct nonzero computation; the table clamp and check_window; TestSplit and
PrepareCase on the reference's configuration values; and the library's argument checks.  No kernel is launched."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests._resize_inputs import A_MAX, A_MIN, CASES, DTYPES, N, SHAPE, blobs, case, inputs, integer_rule_differs, split_config, window_table


def _interpolate_windows(image, labels, rows, resized, out):
    """F.interpolate on the slice of every sample's window, cropped: the reference of the restatement."""
    imgs, labs = [], []
    for s, (start, extent, crop) in enumerate(rows):
        sl = tuple(slice(a, a + e) for a, e in zip(start, extent))
        cr = tuple(slice(c, c + o) for c, o in zip(crop, out))
        imgs.append(F.interpolate(image[s][sl][None, None].double(), size=resized, mode="area")[0, 0][cr])
        labs.append(F.interpolate(labels[s][sl][None, None].float(), size=resized, mode="nearest")[0, 0][cr].long())
    return torch.stack(imgs), torch.stack(labs)


# ---- 1. the restatement against F.interpolate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_equals_interpolate_on_the_windows(tag):
    from transoar_amd.resize import resize_torch
    image, labels = inputs()
    rows, resized, out = CASES[tag]
    table = window_table(rows)
    want, want_lab = _interpolate_windows(image, labels, rows, resized, out)
    got, got_lab = resize_torch(image, labels, table, resized, out, dtype=torch.float64)
    assert got.shape == (N, *out) and got.dtype == torch.float64 and got_lab.dtype == torch.int64
    err = float((got - want).abs().max())
    print("%s: area against interpolate %.3g" % (tag, err))
    assert err <= 1e-12
    assert torch.equal(got_lab, want_lab)
    # the fp32 run (the CPU path of resize) within the project's fp32 bound of the fp64 run; rank 5; labels of every type
    from transoar_amd.resize import resize
    for dtype in DTYPES:
        x, lab = resize(image[:, None], labels[:, None].to(dtype), resized, out, window=table)
        assert x.shape == (N, 1, *out) and x.dtype == torch.float32 and lab.dtype == dtype
        assert float((x[:, 0].double() - want).abs().max() / want.abs().max()) <= 1e-4 and torch.equal(lab[:, 0].long(), want_lab)
    alone, none = resize(image, None, resized, out, window=table)
    assert none is None and torch.equal(alone, x[:, 0])


def test_every_pair_on_a_ramp_and_the_fixture_distinguishes_the_rules():
    """E, R in 1..48 on a 1-D ramp (a (1, 1, 1, E) volume): area within 1e-12 of interpolate in fp64, nearest equal.  At least one
    pair must separate torch's fp32 nearest rule from the integer rule o E // R, and so must every axis of the trap case."""
    from transoar_amd.resize import resize_torch
    worst, separating = 0.0, 0
    for e in range(1, 49):
        ramp = (torch.arange(e, dtype=torch.float64) * 1.37 + 0.11).view(1, 1, 1, e)
        lab = torch.arange(e).view(1, 1, 1, e)
        for r in range(1, 49):
            got, got_lab = resize_torch(ramp, lab, None, (1, 1, r), dtype=torch.float64)
            want = F.interpolate(ramp[None], size=(1, 1, r), mode="area")[0]
            want_lab = F.interpolate(lab[None].float(), size=(1, 1, r), mode="nearest")[0].long()
            worst = max(worst, float((got - want).abs().max()))
            assert torch.equal(got_lab, want_lab), (e, r)
            if not torch.equal(want_lab.view(-1), (torch.arange(r) * e) // r):
                separating += 1
                assert integer_rule_differs(e, r)
    print("worst area error %.3g; %d pairs separate the fp32 nearest rule from the integer rule" % (worst, separating))
    assert worst <= 1e-12
    assert separating >= 1
    (_, extent, _), resized = CASES["trap"][0][0], CASES["trap"][1]
    assert all(integer_rule_differs(e, r) for e, r in zip(extent, resized))
    assert integer_rule_differs(26, 22) and integer_rule_differs(39, 33) and integer_rule_differs(52, 22)


def test_range_scaling_comes_first():
    from transoar_amd.augment import _f32
    from transoar_amd.resize import resize_torch
    image, labels = inputs()
    table, resized, out = case("trap_crop")
    lo, hi = torch.tensor(_f32(A_MIN), dtype=torch.float64), torch.tensor(_f32(A_MAX), dtype=torch.float32)
    v = ((image.double() - lo) / (hi - lo.float()).double()).clamp(0, 1)
    want, _ = resize_torch(v, None, table, resized, out, dtype=torch.float64)
    got, _ = resize_torch(image, None, table, resized, out, A_MIN, A_MAX, dtype=torch.float64)
    assert float((got - want).abs().max()) <= 1e-15
    with pytest.raises(ValueError, match="together"):
        resize_torch(image, None, table, resized, out, a_min=0.0)
    with pytest.raises(ValueError, match="exceed"):
        resize_torch(image, None, table, resized, out, 1.0, 1.0)


# ---- 2. the foreground window -----------------------------------------------------------------------------------------------------
def _window_by_nonzero(lab, classes, margin):
    n, shape = lab.shape[0], lab.shape[1:]
    table = torch.zeros(n, 12, dtype=torch.int32)
    for s in range(n):
        sel = lab[s] > 0 if classes is None else torch.isin(lab[s], torch.tensor(sorted(classes)))
        at = sel.nonzero()
        if at.numel() == 0:
            table[s, 3:6] = torch.tensor(shape)
            continue
        for a in range(3):
            start = max(int(at[:, a].min()) - margin[a], 0)
            end = min(int(at[:, a].max()) + 1 + margin[a], shape[a])
            table[s, a], table[s, 3 + a] = start, end - start
        table[s, 9] = 1
    return table


@pytest.mark.parametrize("classes", [None, (1,), (3, 14), (6, 40), (1, 6, 7, 14, 15), (2, 62)], ids=str)
def test_foreground_window_against_nonzero(classes):
    from transoar_amd.resize import foreground_window, foreground_window_torch
    lab = blobs(n=3, empty=1)
    lab[2, 0, 0, 0], lab[2, SHAPE[0] - 1, SHAPE[1] - 1, SHAPE[2] - 1] = 3, 3          # class 3 touches both borders
    for margin in ((0, 0, 0), (2, 2, 2), (1, 30, 4), (100, 100, 100)):                # the last two clip at both ends
        want = _window_by_nonzero(lab, classes, margin)
        for dtype in DTYPES:
            got = foreground_window_torch(lab.to(dtype), classes, margin)
            assert got.dtype == torch.int32 and torch.equal(got, want), (margin, dtype)
        assert torch.equal(foreground_window(lab[:, None], classes, margin), want)
    assert torch.equal(foreground_window(lab, classes, 2), _window_by_nonzero(lab, classes, (2, 2, 2)))
    want = _window_by_nonzero(lab, classes, (0, 0, 0))
    assert int(want[1, 9]) == 0 and want[1, 3:6].tolist() == list(SHAPE) and want[1, 0:3].tolist() == [0, 0, 0]
    if classes in (None, (3, 14)):
        assert want[2, 0:6].tolist() == [0, 0, 0, *SHAPE] and int(want[2, 9]) == 1
    if classes == (2, 62):
        assert int(want[:, 9].sum()) == 0                                              # nothing selected anywhere
    for bad in ((0,), (63,), (-1,)):
        with pytest.raises(ValueError, match="1..62"):
            foreground_window_torch(lab, bad)
    with pytest.raises(ValueError, match="margin"):
        foreground_window_torch(lab, None, -1)


# ---- 3. the clamp of the table, check_window ---------------------------------------------------------------------------------------
BROKEN = (((-5, 3, 4), (26, 39, 52), (0, 0, 0)), ((0, 3, 4), (26, 39, 52), (0, 0, 0))), \
         (((2, 3, 4), (1000, 39, 52), (0, 0, 0)), ((2, 3, 4), (28, 39, 52), (0, 0, 0))), \
         (((2, 3, 4), (26, 0, -7), (0, 0, 0)), ((2, 3, 4), (26, 1, 1), (0, 0, 0))), \
         (((2, 3, 4), (26, 39, 52), (9, -2, 100)), ((2, 3, 4), (26, 39, 52), (2, 0, 6))), \
         (((99, 43, 4), (26, 39, 52), (0, 0, 0)), ((29, 42, 4), (1, 1, 52), (0, 0, 0)))


@pytest.mark.parametrize("broken,clamped", BROKEN, ids=["start<0", "extent>S", "extent<1", "crop", "start>S-1"])
def test_table_clamp_and_check_window(broken, clamped):
    from transoar_amd.resize import check_window, resize, resize_torch
    image, labels = inputs()
    resized, out = (22, 33, 22), (20, 33, 16)
    good = window_table([clamped, CASES["trap"][0][1]])
    bad = window_table([broken, CASES["trap"][0][1]])
    want, want_lab = resize_torch(image, labels, good, resized, out)
    got, got_lab = resize_torch(image, labels, bad, resized, out)
    assert torch.equal(got, want) and torch.equal(got_lab, want_lab)
    assert check_window(good, SHAPE, resized, out) is good
    with pytest.raises(ValueError, match="window"):
        check_window(bad, SHAPE, resized, out)
    with pytest.raises(ValueError, match="window"):
        resize(image, labels, resized, out, window=bad)                   # a host table is checked, not clamped
    x, lab = resize(image, labels, resized, out, window=good)
    assert torch.equal(x, want) and torch.equal(lab, want_lab)


def test_shape_errors():
    from transoar_amd.resize import resize
    image, labels = inputs()
    with pytest.raises(ValueError, match="does not fit"):
        resize(image, labels, (8, 8, 8), (9, 8, 8))
    with pytest.raises(ValueError, match="labels of shape"):
        resize(image, labels[:, :5], (8, 8, 8))
    with pytest.raises(ValueError, match="window"):
        resize(image, labels, (8, 8, 8), window=torch.zeros(3, 12, dtype=torch.int32))
    out = (torch.empty(N, 8, 9, 10), torch.empty(N, 8, 9, 10, dtype=torch.int64))
    x, lab = resize(image, labels, (8, 9, 10), out=out)
    assert x is out[0] and lab is out[1]
    assert float((x.double() - F.interpolate(image[:, None].double(), size=(8, 9, 10), mode="area")[:, 0]).abs().max()) <= 1e-6


# ---- 4. TestSplit -------------------------------------------------------------------------------------------------------------------
def test_test_split_equals_batch_augment_when_nothing_is_resized():
    """Stored shape == median, no patch: every bin is one voxel, so the split is the range scaling alone and bit-identical to
    BatchAugment(config, 'test', deterministic=True) on the same CPU inputs."""
    from transoar_amd.augment import BatchAugment
    from transoar_amd.resize import TestSplit
    image, labels = inputs()
    cfg = split_config(SHAPE)
    want, want_lab = BatchAugment(cfg, "test", seed=0, deterministic=True)(image, labels.to(torch.int16))
    for deterministic in (True, False):
        got, got_lab = TestSplit(cfg, seed=0, deterministic=deterministic)(image, labels.to(torch.int16))
        assert got.shape == want.shape == (N, 1, *SHAPE) and got.dtype == torch.float32 and got_lab.dtype == torch.int16
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_lab, want_lab)


def test_test_split_resizes_to_the_median_and_crops():
    from transoar_amd.resize import TestSplit, resize_torch
    image, labels = inputs()
    median, patch = (22, 33, 40), (16, 20, 33)
    cfg = split_config(median, patch)
    centred = TestSplit(cfg, seed=0, deterministic=True)
    table = centred.draw(3, SHAPE)
    assert table.dtype == torch.int32 and table[:, 0:3].abs().sum() == 0 and table[:, 3:6].tolist() == [list(SHAPE)] * 3
    assert table[:, 6:9].tolist() == [[3, 6, 3]] * 3 and int(table[:, 10:].abs().sum()) == 0
    x, lab = centred.split(image, labels)
    whole, whole_lab = resize_torch(image, labels, None, median, a_min=A_MIN, a_max=A_MAX)
    assert x.shape == (N, 1, *patch) and lab.shape == x.shape and lab.dtype == torch.int64
    assert torch.equal(x[:, 0], whole[:, 3:19, 6:26, 3:36]) and torch.equal(lab[:, 0], whole_lab[:, 3:19, 6:26, 3:36])
    want = F.interpolate(((image.double() - A_MIN) / (A_MAX - A_MIN)).clamp(0, 1)[:, None], size=median, mode="area")[:, 0]
    assert float((x[:, 0].double() - want[:, 3:19, 6:26, 3:36]).abs().max()) <= 1e-5
    out = (torch.empty(N, 1, *patch), torch.empty(N, 1, *patch, dtype=torch.int64))
    x2, lab2 = centred.split(image, labels, out=out)
    assert x2 is out[0] and lab2 is out[1] and torch.equal(x2, x) and torch.equal(lab2, lab)
    # drawn offsets: seeded, in range, and they vary
    a, b = TestSplit(cfg, seed=4), TestSplit(cfg, seed=4)
    moving = a.draw(200, SHAPE)
    assert torch.equal(moving, b.draw(200, SHAPE)) and not torch.equal(moving, TestSplit(cfg, seed=5).draw(200, SHAPE))
    crops, room = moving[:, 6:9], torch.tensor([6, 13, 7], dtype=torch.int32)
    assert bool((crops >= 0).all()) and bool((crops <= room).all())
    assert len(set(map(tuple, crops.tolist()))) > 50 and bool((crops == room).any(0).all()) and bool((crops == 0).any(0).all())
    with pytest.raises(ValueError, match="does not fit"):
        TestSplit(split_config((10, 10, 10), (16, 8, 8)))


# ---- 5. PrepareCase -----------------------------------------------------------------------------------------------------------------
AMOS = dict(dataset_config="amos", resize_shape=[256, 256, 128], margin=2, key="image", orientation="RAS", min_num_organs=5)
VISCERAL = dict(dataset_config="visceral", resize_shape=[160, 160, 256], margin=5, key="image", orientation="RAS", min_num_organs=12)


def test_prepare_case_from_the_shipped_preprocessing_values():
    """The values of the reference's preprocessing_amos.yaml and preprocessing_visceral.yaml."""
    from transoar_amd.resize import PrepareCase, foreground_window_torch
    amos, visceral = PrepareCase.from_config(AMOS), PrepareCase.from_config(VISCERAL)
    assert amos.resize_shape == (256, 256, 128) and amos.classes == (1, 6, 7, 14, 15) and amos.margin == (2, 2, 2)
    assert visceral.resize_shape == (160, 160, 256) and visceral.classes is None and visceral.margin == (5, 5, 5)
    assert PrepareCase.from_config(dict(AMOS, margin=9)).margin == (2, 2, 2)          # the reference hard-codes [2, 2, 2] for amos
    with pytest.raises(ValueError, match="dataset_config"):
        PrepareCase.from_config(dict(AMOS, dataset_config="kits"))
    # on a toy case: crop to the selected organs' window, then area / nearest to the fixed shape
    lab = blobs()
    image = inputs()[0]
    prep = PrepareCase((12, 14, 16), amos.classes, amos.margin)
    x, y, window = prep(image, lab.to(torch.uint8))
    assert x.shape == (N, 12, 14, 16) and x.dtype == torch.float32 and y.dtype == torch.int32 and y.shape == x.shape
    assert torch.equal(window, foreground_window_torch(lab, amos.classes, 2)) and int(window[:, 9].min()) == 1
    for s in range(N):
        st, ex = window[s, 0:3].tolist(), window[s, 3:6].tolist()
        sl = tuple(slice(a, a + e) for a, e in zip(st, ex))
        assert ex != list(SHAPE)
        want = F.interpolate(image[s][sl][None, None].double(), size=(12, 14, 16), mode="area")[0, 0]
        want_lab = F.interpolate(lab[s][sl][None, None].float(), size=(12, 14, 16), mode="nearest")[0, 0]
        assert float((x[s].double() - want).abs().max()) <= 1e-6 and torch.equal(y[s].float(), want_lab)


# ---- 6. the library's argument checks -------------------------------------------------------------------------------------------------
def test_resize_argument_errors():
    from transoar_amd.resize import lib              # bound from include/transoar_resize.h
    f, w, wb = lib.transoar_resize_forward, lib.transoar_foreground_window, lib.transoar_foreground_window_workspace_bytes
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    F32, U8, I16, I64 = 0, 16, 17, 19
    assert lib.transoar_resize_abi_version() == 1
    ok = (2, 8, 8, 8, 6, 6, 6, 6, 6, 6)               # n, source, resized, out
    # NULL required pointers; labels and labels_out come together; a NULL window is the whole volume (dimensions are looked at next)
    assert f(None, F32, p, U8, *ok, p, 0, 0.0, 1.0, p, p, None) == -1
    assert f(p, F32, p, U8, *ok, p, 0, 0.0, 1.0, None, p, None) == -1
    assert f(p, F32, p, U8, *ok, p, 0, 0.0, 1.0, p, None, None) == -1
    assert f(p, F32, None, U8, *ok, p, 0, 0.0, 1.0, p, p, None) == -1
    # bad dimensions: an extent below 1 or above 2^24, out above the resized grid, too many samples, a sample of 2^40 voxels
    for dims in ((0, 8, 8, 8, 6, 6, 6, 6, 6, 6), (2, 0, 8, 8, 6, 6, 6, 6, 6, 6), (2, 8, 8, 8, 6, 0, 6, 6, 6, 6), (2, 8, 8, 8, 6, 6, 6, 6, 6, -1),
                 (2, 8, 8, 8, 6, 6, 6, 7, 6, 6), (2, 8, 8, 8, 6, 6, 6, 6, 6, 7), (65536, 8, 8, 8, 6, 6, 6, 6, 6, 6),
                 (1, 1 << 14, 1 << 14, 1 << 12, 6, 6, 6, 6, 6, 6), (1, (1 << 24) + 1, 1, 1, 1, 1, 1, 1, 1, 1),
                 (1, 1, 1, 1, 1, 1, (1 << 24) + 1, 1, 1, 1)):
        assert f(p, F32, p, U8, *dims, p, 0, 0.0, 1.0, p, p, None) == -2, dims
    # the range is looked at only when scaling is on
    for lo, hi in ((1.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (0.0, float("inf")), (-3e38, 3e38)):
        assert f(p, F32, p, U8, *ok, p, 1, lo, hi, p, p, None) == -2, (lo, hi)
    # unknown image or label dtype
    assert f(p, 1, p, U8, *ok, p, 0, 0.0, 1.0, p, p, None) == -3
    assert f(p, U8, p, U8, *ok, p, 0, 0.0, 1.0, p, p, None) == -3
    assert f(p, F32, p, 15, *ok, p, 0, 0.0, 1.0, p, p, None) == -3
    assert f(p, I16, p, 20, *ok, p, 0, 0.0, 1.0, p, p, None) == -3
    # pointers not aligned to their element type
    assert f(p + 2, F32, p, U8, *ok, p, 0, 0.0, 1.0, p, p, None) == -4
    assert f(p + 1, I16, p, U8, *ok, p, 0, 0.0, 1.0, p, p, None) == -4
    assert f(p, F32, p, U8, *ok, p + 2, 0, 0.0, 1.0, p, p, None) == -4
    assert f(p, F32, p, U8, *ok, p, 0, 0.0, 1.0, p + 3, p, None) == -4
    assert f(p, F32, p + 4, I64, *ok, p, 0, 0.0, 1.0, p, p, None) == -4
    assert f(p, F32, p, I64, *ok, p, 0, 0.0, 1.0, p, p + 4, None) == -4
    # the foreground window
    need = wb(2, 512)
    assert need == 2 * 6 * 4 and wb(2, 1 << 20) == 2 * 256 * 6 * 4 and wb(0, 512) == 0 and wb(2, 1 << 40) == 0 and wb(65536, 8) == 0
    assert w(None, U8, 2, 8, 8, 8, -1, 0, 0, 0, p, p, need, None) == -1
    assert w(p, U8, 2, 8, 8, 8, -1, 0, 0, 0, None, p, need, None) == -1
    assert w(p, U8, 2, 8, 8, 8, -1, 0, 0, 0, p, None, need, None) == -1
    assert w(p, U8, 2, 0, 8, 8, -1, 0, 0, 0, p, p, need, None) == -2
    assert w(p, U8, 65536, 8, 8, 8, -1, 0, 0, 0, p, p, 1 << 30, None) == -2
    assert w(p, U8, 2, 8, 8, 8, -1, 0, -1, 0, p, p, need, None) == -2
    assert w(p, U8, 1, 1 << 14, 1 << 14, 1 << 12, -1, 0, 0, 0, p, p, 1 << 30, None) == -2
    assert w(p, 15, 2, 8, 8, 8, -1, 0, 0, 0, p, p, need, None) == -3
    assert w(p, U8, 2, 8, 8, 8, -1, 0, 0, 0, p, p, need - 1, None) == -5
    assert w(p + 4, I64, 2, 8, 8, 8, -1, 0, 0, 0, p, p, need, None) == -4
    assert w(p, U8, 2, 8, 8, 8, -1, 0, 0, 0, p + 2, p, need, None) == -4
    assert w(p, U8, 2, 8, 8, 8, -1, 0, 0, 0, p, p + 1, need, None) == -4


def test_dtypes_of_the_tests_are_the_kernel_s():
    from transoar_amd import resize
    assert tuple(resize._LABEL_DT) == DTYPES and tuple(resize._IMAGE_DT) == (torch.float32, torch.int16)
    assert case("trap")[0].shape == (N, 12) == (N, resize.WINDOW)
