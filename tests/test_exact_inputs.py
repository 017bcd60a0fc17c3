"""CPU: the tools of the bit-exact convolution tests (tests/_exact_inputs.py) are themselves right.  The plain fp64 tap-sum
equals F.conv3d in fp64, values and both gradients; the integer generator keeps every reference inside the range where bf16
and fp32 hold integers exactly; the comparison fails at a single changed element and at a single removed (tap, channel)
term -- which the 2^-7-of-the-maximum bound of the tolerance tests lets through on their own Gaussian inputs."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from tests import _exact_inputs as E

HERE = os.path.dirname(os.path.abspath(__file__))


def _table(module, name):
    spec = importlib.util.spec_from_file_location("_exact_table_source", os.path.join(HERE, module + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return getattr(mod, name)


def test_case_tables_are_those_of_the_tolerance_tests():
    assert E.PLAN_CASES == _table("test_conv_plan_gpu", "CASES")
    assert E.GEMM_CASES == _table("test_convgemm_gpu", "CASES")
    assert E.MERGE_SHAPES == _table("test_patch_merge_gpu", "SHAPES")


@pytest.mark.parametrize("shape,stats,routes", E.PLAN_CASES + E.SEAM_CASES)
def test_layer_cases_reach_the_routes_they_name(shape, stats, routes):
    from transoar_amd.conv_plan import plan_conv
    plan = plan_conv(*shape, stats)
    assert (plan.fwd, plan.dgrad if shape[1] != 1 else None, plan.wgrad) == routes


@pytest.mark.parametrize("shape,kernel,pad", [((2, 5, 7, 5, 6, 9, 1), 3, 1), ((1, 6, 4, 7, 5, 9, 2), 3, 1), ((2, 3, 8, 6, 8, 4, 2), 3, 1),
                                              ((2, 4, 8, 5, 6, 7, 2), 2, 0), ((1, 1, 5, 3, 4, 5, 1), 3, 1)])
def test_conv_ref_is_the_fp64_convolution(shape, kernel, pad):
    n, ci, co, d, h, w, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, ci, d, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(co, ci, kernel, kernel, kernel, generator=g, dtype=torch.float64)
    b = torch.randn(co, generator=g, dtype=torch.float64)
    grads = []
    for fn in (lambda a, k, c: E.conv_ref(a, k, c, s, pad, kernel), lambda a, k, c: F.conv3d(a, k, c, stride=s, padding=pad)):
        a, k, c = (t.clone().requires_grad_() for t in (x, wt, b))
        y = fn(a, k, c)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        y.backward(dy)
        grads.append((y.detach(), a.grad, k.grad, c.grad))
    for name, mine, ref in zip(("y", "dx", "dw", "db"), *grads):
        assert mine.shape == ref.shape
        assert float((mine - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name
    # on integers both are exact, so they are equal
    xi, wi = E.ints(x.shape, 0.5, g).double(), E.ints(wt.shape, 0.5, g).double()
    assert torch.equal(E.conv_ref(xi, wi, None, s, pad, kernel), F.conv3d(xi, wi, None, stride=s, padding=pad))


def test_ints_draws_what_it_says():
    g = torch.Generator().manual_seed(0)
    t = E.ints((200, 1000), 0.25, g)
    assert t.dtype == torch.float32 and set(t.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert abs(float((t != 0).float().mean()) - 0.25) < 0.01
    for v in (1.0, 2.0, 3.0):
        assert abs(float((t == v).float().mean()) - 0.25 / 6) < 0.005 and abs(float((t == -v).float().mean()) - 0.25 / 6) < 0.005
    assert E.density(27 * 96) == (40.0 / (27 * 96)) ** 0.5 and E.density(27) == 0.5


_CONV_SHAPES = sorted({c[0] for c in E.PLAN_CASES + E.SEAM_CASES} | {c[:7] for c in E.GEMM_CASES} | set(E.S2_HALO_CASES) | set(E.RING_CASES))


@pytest.mark.parametrize("shape", [s for s in _CONV_SHAPES if E.on_cpu(s)], ids=lambda s: "x".join(map(str, s)))
def test_conv_cases_stay_exactly_representable(shape):
    c = E.conv_case(shape)
    for name in ("y", "y_nobias", "dx"):
        E.assert_bf16_storable(name, getattr(c, name))
    for name in ("dw", "db"):
        E.assert_fp32_storable(name, getattr(c, name))
    assert float(c.y.abs().sum((2, 3, 4)).max()) < E.FP32_EXACT        # the statistics epilogue's per-sample channel sums
    assert float(c.y.abs().max()) > 0 and float(c.dw.abs().max()) > 0
    print(shape, "p = %.3f" % c.p, {k: float(getattr(c, k).abs().max()) for k in ("y", "dx", "dw", "db")})


def test_the_large_cases_are_the_ones_left_to_the_device():
    assert [s for s in _CONV_SHAPES if not E.on_cpu(s)] == [(1, 48, 48, 16, 256, 64, 1), (1, 48, 48, 24, 32, 64, 1), (2, 48, 48, 128, 128, 64, 1)]


@pytest.mark.parametrize("shape", E.MERGE_SHAPES)
def test_merge_cases_stay_exactly_representable(shape):
    c = E.merge_case(shape)
    E.assert_bf16_storable("y", c.y), E.assert_bf16_storable("dx", c.dx), E.assert_fp32_storable("dw", c.dw)
    x64, w64 = c.x.double().requires_grad_(), c.w.double().requires_grad_()
    y = F.conv3d(x64.permute(0, 4, 1, 2, 3), w64, stride=2).permute(0, 2, 3, 4, 1)
    y.backward(c.dy.double())
    assert torch.equal(y.detach(), c.y) and torch.equal(x64.grad, c.dx) and torch.equal(w64.grad, c.dw)


@pytest.mark.parametrize("shape", E.LINEAR_CASES)
def test_linear_cases_stay_exactly_representable(shape):
    E.assert_fp32_storable("dw", E.linear_case(shape).dw)


def test_assert_exact_fails_at_one_changed_element():
    want = E.conv_case((1, 96, 96, 5, 5, 8, 1)).y
    E.assert_exact("y", want.clone().to(torch.bfloat16), want)          # the bf16 store of this reference is exact
    got = want.clone()
    got[0, 37, 4, 0, 7] += 1
    with pytest.raises(AssertionError) as info:
        E.assert_exact("y", got.to(torch.bfloat16), want)
    text = str(info.value)
    assert "1 of %d elements differ" % want.numel() in text and "(0, 37, 4, 0, 7)" in text
    assert "axis 1 (size 96): {37: 1}" in text and "axis 4 (size 8): {7: 1}" in text
    with pytest.raises(AssertionError):
        E.assert_exact("y", want[:, :-1], want)


def _drop_one_term(x, w, y, voxel, co, pick):
    """y with one (tap, channel) term of output channel co at `voxel` removed; pick(products (27 Cin,)) -> index of the
    term.  -> (y', the term's value, the voxel's products)"""
    d, h, wd = voxel
    xp = F.pad(x, (1, 1) * 3)
    window = xp[0, :, d:d + 3, h:h + 3, wd:wd + 3].reshape(x.shape[1], 27).t()             # (27, Cin)
    products = (window * w[co].reshape(w.shape[1], 27).t()).reshape(-1)
    flat = pick(products)
    out = y.clone()
    out[0, co, d, h, wd] -= products[flat]
    return out, float(products[flat]), products


def _live(products):
    return products.nonzero().view(-1)              # not a padding tap (and, on the sparse integers, both factors nonzero)


def _median_term(products):
    live = _live(products)
    return int(live[products[live].abs().argsort()[live.numel() // 2]])


def test_one_dropped_term_passes_the_tolerance_bound_and_fails_assert_exact():
    """The Cin = 96 case, one (tap, channel) term removed at a corner voxel of the volume.  On the Gaussian inputs of the
    tolerance tests the 2^-7-of-the-maximum comparison passes (it would for any term of up to 2^-7 max|y|: here that is most
    of them); on the integer inputs the comparison is exact and fails, naming the voxel."""
    n, ci, co, d, h, w, s = shape = (1, 96, 96, 5, 5, 8, 1)
    g = torch.Generator().manual_seed(96)
    x = torch.randn(n, ci, d, h, w, generator=g).to(torch.bfloat16).double()
    wt = (torch.randn(co, ci, 3, 3, 3, generator=g) * 0.1).to(torch.bfloat16).double()
    y = E.conv_ref(x, wt, None, s, 1, 3)
    bad, term, products = _drop_one_term(x, wt, y, (0, 0, 0), 5, _median_term)
    bound = 2.0 ** -7 * float(y.abs().max())
    unseen = float((products[_live(products)].abs() <= bound).float().mean())
    print("gaussian: term %.4f, max|y| %.2f, rel %.5f against 2^-7 = %.5f; %.0f %% of this voxel's terms are under the bound"
          % (term, float(y.abs().max()), E.rel_to_max(bad, y), 2.0 ** -7, 100 * unseen))
    assert term != 0 and E.rel_to_max(bad, y) <= 2.0 ** -7
    assert unseen > 0.5                             # "most of them"
    with pytest.raises(AssertionError):
        E.assert_exact("y", bad, y)

    c = E.conv_case(shape)
    bad, term, _ = _drop_one_term(c.x.double(), c.w.double(), c.y_nobias, (0, 0, 0), 5, lambda p: int(_live(p)[0]))
    print("integer: term %g, max|y| %g, rel %.5f" % (term, float(c.y_nobias.abs().max()), E.rel_to_max(bad, c.y_nobias)))
    assert abs(term) >= 1
    with pytest.raises(AssertionError) as info:
        E.assert_exact("y", bad.to(torch.bfloat16), c.y_nobias)
    assert "1 of %d elements differ" % c.y.numel() in str(info.value) and "(0, 5, 0, 0, 0)" in str(info.value)
