"""Integer inputs on which the convolution kernels must equal an fp64 reference BIT FOR BIT, the plain reference itself, and
the comparison that names where a mismatch lies (tests/test_exact_inputs.py, tests/test_conv_exact_gpu.py).

Every convolution kernel multiplies bf16 operands and accumulates in fp32 (include/transoar_conv3d.h,
include/transoar_convgemm.h, include/transoar_patchmerge.h).  With small integers every product and every partial sum is an
integer, exact in any summation order; the bf16 store is exact while |y| <= 256 and an fp32 result below 2^24.  So one wrong,
missing or doubled (tap, channel) term anywhere is a differing element, where the 2^-7-of-the-maximum bound on Gaussian
inputs cannot see it from 48 channels up (README, "How parity is stated").

References are computed once per process and never modified."""
import functools
from types import SimpleNamespace

import torch

BF16_EXACT = 256.0             # integers up to 2^8 are bf16 numbers (8 significand bits)
FP32_EXACT = float(1 << 24)    # integers below 2^24 are fp32 numbers, and so is every partial sum of terms whose |.| sum to less

# ---- case tables.  The first four repeat the tables of the tolerance tests of the same kernels (test_exact_inputs.py
# checks that they still agree); the others are the seams those tests reach only at flagship size.
# ((N, Cin, Cout, D, H, W, stride), with statistics, (fwd, dgrad, wgrad)): tests/test_conv_plan_gpu.py::CASES
PLAN_CASES = [
    ((2, 24, 24, 3, 4, 64, 1), False, ("direct", "direct_flipped", "lds_tr")),
    ((1, 1, 24, 18, 30, 128, 1), False, ("c1_halo", None, "c1_tr")),
    ((1, 1, 8, 2, 3, 48, 1), False, ("c1_padded", None, "c1")),
    ((1, 24, 24, 18, 22, 200, 1), True, ("stats_halo", "direct_flipped", "voxel_major")),
    ((1, 96, 96, 5, 5, 8, 1), False, ("igemm", "igemm_s1", "voxel_major")),
    ((1, 48, 48, 24, 32, 64, 1), False, ("igemm", "igemm_s1", "voxel_major")),
    ((1, 24, 48, 8, 8, 16, 2), False, ("igemm", "s2_halo", "voxel_major")),
    ((2, 48, 96, 4, 6, 16, 2), False, ("igemm", "s2_classes", "voxel_major")),
    ((1, 48, 48, 16, 256, 64, 1), False, ("igemm", "igemm_s1", "ring")),
    ((2, 48, 48, 128, 128, 64, 1), False, ("igemm", "igemm_s1", "lds_tr")),     # 2^21 rows: TWO_RANGE_CASE below
    ((1, 1, 40, 2, 3, 16, 1), False, ("c1_padded", None, "channels_first")),
]
TWO_RANGE_CASE = PLAN_CASES[9]
LAYER_CASES = [c for c in PLAN_CASES if c is not TWO_RANGE_CASE]
# (N, Cin, Cout, D, H, W, stride, bias): tests/test_convgemm_gpu.py::CASES
GEMM_CASES = [
    (2, 48, 48, 6, 10, 16, 1, False), (1, 24, 48, 8, 8, 16, 2, False), (2, 48, 96, 4, 6, 16, 2, False),
    (1, 96, 96, 5, 5, 8, 1, False), (1, 96, 384, 4, 4, 8, 1, True), (2, 8, 40, 3, 7, 24, 1, True),
    (1, 192, 136, 3, 5, 7, 1, True), (1, 200, 64, 5, 7, 9, 2, False), (1, 384, 768, 2, 4, 4, 2, False),
    (1, 768, 768, 2, 2, 4, 1, False), (2, 96, 192, 6, 6, 8, 2, False), (1, 56, 72, 7, 9, 11, 2, True),
]
# (B, D, H, W, C): tests/test_patch_merge_gpu.py::SHAPES
MERGE_SHAPES = [(1, 2, 2, 2, 16), (2, 5, 6, 7, 48), (1, 4, 6, 70, 32), (2, 2, 4, 4, 96), (1, 2, 2, 4, 768)]
S2_HALO_CASES = [(2, 24, 48, 7, 9, 15, 2), (1, 24, 48, 260, 8, 16, 2)]      # D > 255: the piece table's 'no piece' marker
RING_CASES = [(2, 48, 48, 5, 9, 128, 1), (1, 56, 40, 7, 11, 127, 2), (1, 8, 40, 9, 40, 255, 2)]
LINEAR_CASES = [(1000, 384, 384), (333, 1024, 384)]                         # (T, K, N)
# the Cin = 1 routes PLAN_CASES does not reach (c1_tr at W = 64 and W = 256, c1 over three samples) and the halo-tile forward
# with a partial tile on each axis, with and without the statistics epilogue
SEAM_CASES = [
    ((2, 1, 24, 5, 7, 64, 1), False, ("c1_padded", None, "c1_tr")),
    ((1, 1, 32, 4, 6, 256, 1), False, ("c1_padded", None, "c1_tr")),
    ((1, 1, 16, 6, 4, 256, 1), False, ("c1_padded", None, "c1_tr")),
    ((3, 1, 24, 5, 3, 16, 1), False, ("c1_padded", None, "c1")),
    ((1, 8, 32, 20, 30, 120, 1), False, ("direct", "direct_flipped", "voxel_major")),
    ((1, 8, 32, 20, 30, 120, 1), True, ("stats_halo", "direct_flipped", "voxel_major")),
    ((2, 16, 24, 17, 33, 136, 1), False, ("direct", "direct_flipped", "voxel_major")),
    ((2, 16, 24, 17, 33, 136, 1), True, ("stats_halo", "direct_flipped", "voxel_major")),
]
CPU_MACS = 1 << 31          # references of up to this many multiply-adds are computed on the CPU, larger ones on the device


def density(k):
    """Probability of a nonzero entry for a layer whose largest contraction length is k: the variance of a sum of k products
    is k p^2 (14/3)^2 <= 40 (14/3)^2 = 871, so 256 is 8.7 standard deviations away."""
    return min(0.5, (40.0 / k) ** 0.5)


def ints(shape, p, generator):
    """fp32 tensor on the generator's device: each entry nonzero with probability p, nonzeros uniform on {+-1, +-2, +-3}."""
    dev = generator.device
    mag = torch.randint(1, 4, shape, generator=generator, device=dev, dtype=torch.int8)
    sign = torch.randint(0, 2, shape, generator=generator, device=dev, dtype=torch.int8) * 2 - 1
    keep = torch.rand(shape, generator=generator, device=dev) < p
    return (mag * sign * keep).float()


def out_size(size, stride, pad, kernel):
    return (size + 2 * pad - kernel) // stride + 1


def conv_ref(x, w, bias, stride, pad, kernel):
    """x (N, Cin, D, H, W), w (Cout, Cin, k, k, k), bias (Cout,) or None, all fp64 -> y (N, Cout, Do, Ho, Wo) fp64: the sum
    over the taps of (strided slice of the padded input) @ w[:, :, tap].T.  Differentiable; no convolution routine."""
    xp = torch.nn.functional.pad(x.permute(0, 2, 3, 4, 1), (0, 0) + (pad, pad) * 3)
    od, oh, ow = (out_size(v, stride, pad, kernel) for v in x.shape[2:])
    y = None
    for kd in range(kernel):
        for kh in range(kernel):
            for kw in range(kernel):
                src = xp[:, kd:kd + stride * (od - 1) + 1:stride, kh:kh + stride * (oh - 1) + 1:stride,
                         kw:kw + stride * (ow - 1) + 1:stride]
                term = src @ w[:, :, kd, kh, kw].t()
                y = term if y is None else y + term
    if bias is not None:
        y = y + bias
    return y.permute(0, 4, 1, 2, 3)


def macs(shape, kernel=3, pad=1):
    n, ci, co, d, h, w, s = shape
    return n * out_size(d, s, pad, kernel) * out_size(h, s, pad, kernel) * out_size(w, s, pad, kernel) * ci * co * kernel ** 3


def on_cpu(shape, kernel=3, pad=1):
    return macs(shape, kernel, pad) <= CPU_MACS


def conv_case(shape, kernel=3, pad=1):
    """shape (N, Cin, Cout, D, H, W, stride) -> x (N, Cin, D, H, W), w (Cout, Cin, k, k, k), b (Cout,), dy: integer-valued
    fp32; y, y_nobias, dx, dw, db: the fp64 reference.  Drawn and computed on the CPU up to CPU_MACS and kept; on the device
    above, and not kept (each such case has one test, and the largest holds 3 GB)."""
    return (_kept_conv_case if on_cpu(shape, kernel, pad) else _conv_case)(shape, kernel, pad)


def _conv_case(shape, kernel, pad):
    n, ci, co, d, h, w, s = shape
    dev = "cpu" if on_cpu(shape, kernel, pad) else "cuda"
    g = torch.Generator(device=dev).manual_seed(sum((i + 1) * v for i, v in enumerate(shape)) + 1000 * kernel)
    p = density(kernel ** 3 * max(ci, co))
    c = SimpleNamespace(p=p, device=dev)
    c.x = ints((n, ci, d, h, w), p, g)
    c.w = ints((co, ci) + (kernel,) * 3, p, g)
    c.b = ints((co,), p, g)
    c.dy = ints((n, co) + tuple(out_size(v, s, pad, kernel) for v in (d, h, w)), p, g)
    x64, w64, b64 = (t.double().requires_grad_() for t in (c.x, c.w, c.b))
    ys = []
    for i in range(n):          # sample by sample: the graph of one sample is freed before the next one is built
        y = conv_ref(x64[i:i + 1], w64, b64, s, pad, kernel)
        y.backward(c.dy[i:i + 1].double())
        ys.append(y.detach())
    c.y = torch.cat(ys)
    c.y_nobias = c.y - b64.detach().view(1, -1, 1, 1, 1)
    c.dx, c.dw, c.db = x64.grad, w64.grad, b64.grad
    return c


_kept_conv_case = functools.lru_cache(maxsize=None)(_conv_case)


@functools.lru_cache(maxsize=None)
def merge_case(shape):
    """Patch merging (k = s = 2, no padding, no bias) on the token map (B, D, H, W, C) as it lies: x, w (2C, C, 2, 2, 2),
    dy (B, D/2, H/2, W/2, 2C) integer-valued fp32 and the fp64 reference y, dx (both channels-last like x and dy), dw."""
    b, d, h, w, ch = shape
    g = torch.Generator().manual_seed(sum((i + 1) * v for i, v in enumerate(shape)))
    p = density(8 * 2 * ch)
    c = SimpleNamespace(p=p, device="cpu")
    c.x = ints(shape, p, g)
    c.w = ints((2 * ch, ch, 2, 2, 2), p, g)
    c.dy = ints((b, d // 2, h // 2, w // 2, 2 * ch), p, g)
    x64, w64 = c.x.double().requires_grad_(), c.w.double().requires_grad_()
    y = conv_ref(x64.permute(0, 4, 1, 2, 3), w64, None, 2, 0, 2).permute(0, 2, 3, 4, 1)
    y.backward(c.dy.double())
    c.y, c.dx, c.dw = y.detach(), x64.grad, w64.grad
    return c


@functools.lru_cache(maxsize=None)
def linear_case(shape):
    """(T, K, N) -> x (T, K), dy (T, N) integer-valued fp32, dw (N, K) fp64 = dy^T x."""
    t, k, nn_ = shape
    g = torch.Generator().manual_seed(t + 3 * k + 7 * nn_)
    c = SimpleNamespace(p=density(t), device="cpu")
    c.x, c.dy = ints((t, k), c.p, g), ints((t, nn_), c.p, g)
    c.dw = c.dy.double().t() @ c.x.double()
    return c


def assert_bf16_storable(name, ref):
    """The precondition of an exact comparison of a bf16 result: stated on the reference alone."""
    top = float(ref.abs().max())
    assert top <= BF16_EXACT, "%s: max |reference| = %g > 256: lower the density of this case" % (name, top)


def assert_fp32_storable(name, ref):
    top = float(ref.abs().max())
    assert top < FP32_EXACT, "%s: max |reference| = %g >= 2^24: lower the density of this case" % (name, top)


def mismatch_report(name, got, want, first=8, bins=24):
    """What differs and where: count, the first index tuples with both values, and per axis how many differing elements lie
    at each index (a face, a tile seam or a channel block shows as a few populated indices)."""
    idx = (got != want).nonzero()
    lines = ["%s: %d of %d elements differ, shape %s" % (name, idx.shape[0], want.numel(), tuple(want.shape))]
    for row in idx[:first].tolist():
        lines.append("  %s: got %r, want %r" % (tuple(row), float(got[tuple(row)]), float(want[tuple(row)])))
    for axis in range(want.dim()):
        counts = torch.bincount(idx[:, axis], minlength=want.shape[axis]).tolist()
        hit = [(i, c) for i, c in enumerate(counts) if c]
        shown = ", ".join("%d: %d" % ic for ic in hit[:bins]) + (", ... (%d indices)" % len(hit) if len(hit) > bins else "")
        lines.append("  axis %d (size %d): {%s}" % (axis, want.shape[axis], shown))
    return "\n".join(lines)


def assert_exact(name, got, want):
    """got (any dtype, any device) == want (fp64) element for element."""
    assert want.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    got = got.detach().to(want.device).double()
    if not torch.equal(got, want):
        raise AssertionError(mismatch_report(name, got, want))


def rel_to_max(got, want):
    """The yardstick of the tolerance tests: max|a - b| / max|b|."""
    return float((got.double() - want.double()).abs().max()) / float(want.double().abs().max())
