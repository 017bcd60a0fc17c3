"""GPU: every route of the 3x3x3 convolution (conv_plan.plan_conv) and the convolutional patch merging, BIT FOR BIT against
an fp64 reference on small-integer inputs (tests/_exact_inputs.py).  The kernels multiply bf16 operands and accumulate in
fp32 -- split-K partial maps, partial tiles and atomics included -- so on integers every product and partial sum is exact in
any order, the bf16 store is exact up to 256 and the fp32 gradients below 2^24: one wrong, missing or doubled (tap, channel)
term is a differing element, and the failure message says where they lie.  Each test first asserts, on the reference alone,
that it is inside that range.  The tolerance tests of the same kernels (test_conv3d_gpu, test_convgemm_gpu,
test_conv_plan_gpu, test_patch_merge_gpu) bound the rounding; these pin the indexing."""
import pytest
import torch

from tests import _exact_inputs as E

pytestmark = pytest.mark.gpu
CL3D = torch.channels_last_3d


def _id(shape):
    return "x".join(map(str, shape))


def _layer_ids(cases):
    return [_id(c[0]) + ("-stats" if c[1] else "") for c in cases]


def _dev_bf16(t, channels_last=True):
    t = t.cuda().to(torch.bfloat16)
    return t.contiguous(memory_format=CL3D) if channels_last else t.contiguous()


def _check(c, results, bf16=("y", "y_nobias", "dx"), fp32=("dw", "db")):
    """results: {name of the reference: kernel output}.  The preconditions first, on the reference alone."""
    for name in results:
        ref = getattr(c, name)
        assert name in bf16 + fp32
        (E.assert_bf16_storable if name in bf16 else E.assert_fp32_storable)(name, ref)
    for name, got in results.items():
        assert got.dtype == (torch.bfloat16 if name in bf16 else torch.float32), (name, got.dtype)
        E.assert_exact(name, got, getattr(c, name))


def _run_layer(shape, stats, routes):
    """One layer through Conv3dK3 with integer weights and bias: y, dx, dW, db exact; with statistics, the same y and the
    exact per-sample channel sums."""
    from transoar_amd import conv3d
    from transoar_amd.conv_plan import plan_conv
    n, ci, co, d, h, w, s = shape
    plan = plan_conv(*shape, stats)
    assert (plan.fwd, plan.dgrad if ci != 1 else None, plan.wgrad) == routes
    assert conv3d.Conv3dK3.enabled and conv3d.Conv3dK3.min_voxels == 0
    c = E.conv_case(shape)
    conv = conv3d.Conv3dK3(ci, co, 3, stride=s, padding=1, bias=True).cuda()
    conv.weight.data.copy_(c.w)
    conv.bias.data.copy_(c.b)
    x = _dev_bf16(c.x, channels_last=ci != 1).requires_grad_(ci != 1)
    if stats:
        y, part = conv.forward_with_stats(x)
        assert part is not None and tuple(part.shape) == (plan.stat_rows, 2, 32)
    else:
        y = conv(x)
    assert y.is_contiguous(memory_format=CL3D)
    y.backward(_dev_bf16(c.dy))
    results = {"y": y, "dw": conv.weight.grad, "db": conv.bias.grad}
    if ci != 1:
        results["dx"] = x.grad
    _check(c, results)
    if stats:
        # every partial sum of a channel is an integer below sum |y| < 2^24: exact in fp32, whatever the order
        assert float(c.y.abs().sum((2, 3, 4)).max()) < E.FP32_EXACT
        got = part.view(n, plan.stat_rows // n, 2, 32).double().sum(1).cpu()
        E.assert_exact("channel sums", got[:, 0, :co], c.y.sum((2, 3, 4)).cpu())
        want_sq = (c.y ** 2).sum((2, 3, 4)).cpu()                       # above 2^24: the bound of tests/test_instnorm_gpu.py
        assert ((got[:, 1, :co] - want_sq).abs() <= 2e-6 * want_sq).all()
        assert float(got[:, :, co:].abs().sum()) == 0.0                 # (no such column at 32 channels)


# ---- a. one case per route of plan_conv
@pytest.mark.parametrize("shape,stats,routes", E.LAYER_CASES, ids=_layer_ids(E.LAYER_CASES))
def test_every_planned_route_is_exact(shape, stats, routes):
    _run_layer(shape, stats, routes)


# ---- b. straight through conv_gemm
@pytest.mark.parametrize("case", E.GEMM_CASES, ids=_id)
@pytest.mark.parametrize("split", [None, 1, 3])
def test_conv_gemm_is_exact(case, split):
    from transoar_amd import conv_gemm as G
    shape, bias = case[:7], case[7]
    n, ci, co, d, h, w, s = shape
    c = E.conv_case(shape)
    x, g = _dev_bf16(c.x), _dev_bf16(c.dy)
    wt, b = c.w.cuda(), c.b.cuda()
    results = {"y": G.conv_forward(x, G.pack_fwd(wt), b, s, split=split),
               "dx": G.conv_dgrad(g, G.pack_dgrad(wt), s, (d, h, w), split=split),
               "dw": G.conv_wgrad(x, g, s)}
    if not bias:                                    # the table's own setting too: no bias pointer
        results["y_nobias"] = G.conv_forward(x, G.pack_fwd(wt), None, s, split=split)
    _check(c, results)


@pytest.mark.parametrize("shape", E.S2_HALO_CASES, ids=_id)
def test_stride2_dgrad_halo_and_parity_classes_are_exact(shape):
    from transoar_amd import conv_gemm as G
    from transoar_amd.conv_plan import dgrad_gemm
    n, ci, co, d, h, w, s = shape
    assert G.DGRAD_S2_HALO and dgrad_gemm(n, ci, co, d, h, w, s)[0] == "s2_halo"
    assert dgrad_gemm(n, ci, co, d, h, w, s, general=True)[0] == "s2_classes"
    c = E.conv_case(shape)
    g, wkt = _dev_bf16(c.dy), G.pack_dgrad(c.w.cuda())
    _check(c, {"dx": G.conv_dgrad(g, wkt, s, (d, h, w))})
    _check(c, {"dx": G.conv_dgrad(g, wkt, s, (d, h, w), split=1)})


@pytest.mark.parametrize("shape", E.RING_CASES, ids=_id)
@pytest.mark.parametrize("chunks", [None, 3])
def test_weight_gradient_ring_is_exact(shape, chunks):
    from transoar_amd import conv_gemm as G
    c = E.conv_case(shape)
    assert c.dy.shape[-1] % 64 == 0
    _check(c, {"dw": G.conv_wgrad_ring(_dev_bf16(c.x), _dev_bf16(c.dy), shape[6], chunks=chunks)})


@pytest.mark.parametrize("shape", E.LINEAR_CASES, ids=_id)
def test_linear_wgrad_is_exact(shape):
    from transoar_amd import conv_gemm as G
    c = E.linear_case(shape)
    _check(c, {"dw": G.linear_wgrad(c.x.cuda().to(torch.bfloat16), c.dy.cuda().to(torch.bfloat16))})


# ---- c. the seams the Gaussian-input tests reach only at flagship size
def test_two_batch_ranges_and_four_lds_blocks_are_exact():
    """2 x 128 x 128 x 64 = 2^21 rows: two batch ranges forward and backward, the LDS weight gradient in four 32-channel
    blocks.  The reference is computed on the device in fp64 (sample by sample) and takes most of this test's time."""
    from transoar_amd.conv_plan import plan_conv
    shape, stats, routes = E.TWO_RANGE_CASE
    plan = plan_conv(*shape, stats)
    assert len(plan.fwd_ranges) == 2 and len(plan.dgrad_ranges) == 2 and len(plan.wgrad_blocks) == 4
    assert not E.on_cpu(shape)
    _run_layer(shape, stats, routes)


@pytest.mark.parametrize("shape,stats,routes", E.SEAM_CASES, ids=_layer_ids(E.SEAM_CASES))
def test_one_channel_routes_and_partial_halo_tiles_are_exact(shape, stats, routes):
    _run_layer(shape, stats, routes)


# ---- d. patch merging
@pytest.mark.parametrize("shape", E.MERGE_SHAPES, ids=_id)
def test_patch_merge_is_exact(shape):
    from transoar_amd import patch_merge
    b, d, h, w, ch = shape
    c = E.merge_case(shape)
    x = c.x.cuda().to(torch.bfloat16).requires_grad_()
    weight = c.w.cuda().requires_grad_()
    y = patch_merge.patch_merge_conv(x, weight)
    y.backward(c.dy.cuda().to(torch.bfloat16))
    _check(c, {"y": y, "dx": x.grad, "dw": weight.grad})
    dx = x.grad
    assert bool((dx[:, d // 2 * 2:] == 0).all()) and bool((dx[:, :, h // 2 * 2:] == 0).all()) and bool((dx[:, :, :, w // 2 * 2:] == 0).all())
    assert bool((dx != 0).any())
