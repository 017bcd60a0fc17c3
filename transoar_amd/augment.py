"""Batch augmentation on the device (include/transoar_augment.h, csrc/augment.hip): what the reference does for every batch on host
workers -- TransoarDataset.__getitem__ -> get_transforms('train') of transoar/data/transforms.py:76-165, a MONAI chain that resamples
each volume several times in a row -- as ONE launch per batch: intensity range scaling, one trilinear resample of the volume
(nearest for its label map) through a per-sample affine map, and an intensity gain / offset.

Built: ScaleIntensityRanged, RandRotated, RandZoomd, RandAffined (translate), the three RandFlipd, RandSpatialCropd,
RandScaleIntensityd and RandShiftIntensityd -- the steps the two shipped YAMLs switch on (and the flips, which are sign changes in
the same matrix).  The four steps both YAMLs switch off -- RandGaussianNoised, RandGaussianSmoothd, RandAdjustContrastd and the
shear RandAffined -- are opt-in: BatchAugment(..., full_chain=True).  Without it p_gaussian_noise, p_gaussian_smooth,
p_adjust_contrast and p_shear above 0 raise a ValueError that names the key.  Shear is one more factor of the affine map
(compose_params(shear=...)); the other three are the intensity tail, a launch sequence of its own after the resample
(transoar_augment_intensity: intensity_into, its table from compose_intensity, its specification in torch intensity_torch).
The order of the six shear coefficients and their padding with zeros are MONAI's create_shear as remembered: MONAI is not
installed, so neither can be checked here (with the YAMLs' symmetric ranges the distribution does not depend on the sign).

Two deliberate differences from the reference:
  * the spatial steps are composed into one affine map per sample and the volume is interpolated ONCE, trilinear; the reference
    interpolates after every step and zooms in `area` mode;
  * the parameters are drawn by this project's own seeded generator (a CPU torch.Generator), not MONAI's random stream.
MONAI's Euler convention cannot be checked without MONAI; with the symmetric angle ranges of the YAMLs the distribution of the
maps does not depend on it.

The table (N, 16) fp32 and the operation are specified in include/transoar_augment.h.  `augment_torch` is that specification in
batched torch with explicit index arithmetic (no grid_sample): the path for CPU tensors, for inputs the kernel does not take and
for TRANSOAR_AUGMENT_HIP=0, and with dtype=torch.float64 the reference of the tests.  a_min and a_max are rounded to fp32 first
in every path: the C ABI takes them as floats.
"""
import math
import os

import torch

from . import _native

lib = _native.bind("augment", abi=1)
ENABLED = os.environ.get("TRANSOAR_AUGMENT_HIP", "1") != "0"
PARAMS = 16
MAX_COORD = float(2 ** 24)
_LABEL_DT = {torch.uint8: 16, torch.int16: 17, torch.int32: 18, torch.int64: 19}
UNSUPPORTED = ("p_gaussian_noise", "p_gaussian_smooth", "p_adjust_contrast", "p_shear")     # without full_chain=True
TAIL_WORDS = 12
NOISE, SMOOTH, CONTRAST = 1, 2, 4
MAX_SIGMA = 4.0


def _volume(t, what):
    """(N, 1, D, H, W) or (N, D, H, W) -> (N, D, H, W)"""
    if not torch.is_tensor(t) or t.dim() not in (4, 5) or (t.dim() == 5 and t.shape[1] != 1):
        raise ValueError("%s: a tensor of shape (N, 1, D, H, W) or (N, D, H, W), got %s"
                         % (what, str(tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    return t[:, 0] if t.dim() == 5 else t


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def _check_shapes(img, lab, params, out_shape):
    n = img.shape[0]
    out_shape = tuple(int(s) for s in out_shape)
    if len(out_shape) != 3 or any(o < 1 or o > s for o, s in zip(out_shape, img.shape[1:])):
        raise ValueError("out_shape %s: three extents, each between 1 and the input's %s" % (out_shape, tuple(img.shape[1:])))
    if lab is not None and lab.shape != img.shape:
        raise ValueError("labels of shape %s for an image of shape %s" % (tuple(lab.shape), tuple(img.shape)))
    if not torch.is_tensor(params) or params.shape != (n, PARAMS):
        raise ValueError("params: a tensor of shape (%d, %d)" % (n, PARAMS))
    return out_shape


def check_table(params):
    """Refuse a table the kernel would treat as 'everything outside': an entry of [M | t] that is not finite or beyond +-2^24,
    or a gain / offset that is not finite.  Host tables only (a device table is not read back)."""
    p = params.detach().to(torch.float64)
    if p.dim() != 2 or p.shape[1] != PARAMS:
        raise ValueError("params: a table of shape (N, %d), got %s" % (PARAMS, tuple(p.shape)))
    if not bool(torch.isfinite(p).all()) or float(p[:, :12].abs().max()) > MAX_COORD:
        raise ValueError("params: every entry must be finite and the map's entries within +-2^24")
    return params


def usable(image, labels=None):
    """Can the kernel take these inputs?"""
    ok = (ENABLED and torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.dim() in (4, 5)
          and image.numel() > 0 and image.shape[0] <= 65535)
    if ok and labels is not None:
        ok = torch.is_tensor(labels) and labels.is_cuda and labels.dtype in _LABEL_DT and labels.device == image.device
    return bool(ok)


def augment_into(image, labels, params, image_out, labels_out, a_min, a_max):
    """The kernel on the current stream: image (N, [1,] Di, Hi, Wi) fp32, labels the same shape or None, params a DEVICE table
    (N, 16) fp32 -> image_out (N, [1,] Do, Ho, Wo) fp32 and labels_out in place.  Capturable; nothing is read back."""
    img, out = _volume(image, "image"), _volume(image_out, "image_out")
    lab = None if labels is None else _volume(labels, "labels")
    lout = None if labels_out is None else _volume(labels_out, "labels_out")
    _check_shapes(img, lab, params, out.shape[1:])
    assert usable(img, lab), "augment_into: fp32 CUDA image (and uint8 / int16 / int32 / int64 CUDA labels)"
    assert img.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == img.shape[0]
    assert params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()
    assert (lab is None) == (lout is None)
    if lab is not None:
        assert lab.is_contiguous() and lout.is_contiguous() and lout.dtype == lab.dtype and lout.shape == out.shape
    n, di, hi, wi = img.shape
    _native.launch(lib.transoar_augment_forward, img, img.data_ptr(), _native.ptr(lab), _LABEL_DT[lab.dtype] if lab is not None else 0,
                   n, di, hi, wi, out.shape[1], out.shape[2], out.shape[3], params.data_ptr(), float(a_min), float(a_max),
                   out.data_ptr(), _native.ptr(lout))


def augment(image, labels, params, out_shape, a_min, a_max, out=None):
    """-> (image (N, [1,] Do, Ho, Wo) fp32, labels or None), in the rank of the inputs.  params: the table (N, 16) fp32; a HOST
    table is checked (check_table) and uploaded, a device table is taken as it is.  out=(image_out, labels_out) writes in place.
    CUDA inputs go through the kernel, anything else (and TRANSOAR_AUGMENT_HIP=0) through augment_torch."""
    img = _volume(image, "image")
    lab = None if labels is None else _volume(labels, "labels")
    out_shape = _check_shapes(img, lab, params, out_shape)
    if not params.is_cuda:
        check_table(params)
    if not usable(img, lab):
        got = augment_torch(image, labels, params.to(img.device), out_shape, a_min, a_max)
        if out is not None:
            out[0].copy_(got[0].view_as(out[0]))
            if lab is not None:
                out[1].copy_(got[1].view_as(out[1]))
            return out[0], (out[1] if lab is not None else None)
        return got
    lead = image.shape[:image.dim() - 3]
    if out is None:
        out = (torch.empty(*lead, *out_shape, dtype=torch.float32, device=img.device),
               None if lab is None else torch.empty(*labels.shape[:labels.dim() - 3], *out_shape, dtype=lab.dtype, device=img.device))
    table = params.to(device=img.device, dtype=torch.float32, non_blocking=True).contiguous()
    augment_into(image.contiguous(), None if lab is None else labels.contiguous(), table, out[0], None if lab is None else out[1],
                 a_min, a_max)
    return out[0], (out[1] if lab is not None else None)


def augment_torch(image, labels, params, out_shape, a_min, a_max, dtype=torch.float32):
    """The specification of include/transoar_augment.h in batched torch on the inputs' device: explicit index arithmetic, every
    corner gathered from a clamped address and selected by torch.where.  The source coordinates, their floor and fraction are
    always fp64 (as in the kernel); the weights, the range scaling, the sum and gain / offset are in `dtype`.  With torch.float64
    it is the reference of the tests.  -> (image in `dtype`, labels or None), in the rank of the inputs."""
    img = _volume(image, "image")
    lab = None if labels is None else _volume(labels, "labels")
    do, ho, wo = _check_shapes(img, lab, params, out_shape)
    n, di, hi, wi = img.shape
    dev = img.device
    p32 = params.to(device=dev, dtype=torch.float32)
    p64 = p32.to(torch.float64)
    lo = torch.tensor(_f32(a_min), dtype=dtype, device=dev)
    rng = (torch.tensor(_f32(a_max), dtype=torch.float32, device=dev) - lo.to(torch.float32)).to(dtype)       # the kernel's fp32 range
    v = ((img.to(dtype) - lo) / rng).clamp(0, 1).reshape(n, -1)
    grid = [torch.arange(s, dtype=torch.float64, device=dev).view(shape) for s, shape in
            ((do, (1, -1, 1, 1)), (ho, (1, 1, -1, 1)), (wo, (1, 1, 1, -1)))]
    col = lambda k: p64[:, k].view(n, 1, 1, 1)
    s = [col(4 * a + 2) * grid[2] + (col(4 * a + 1) * grid[1] + (col(4 * a) * grid[0] + col(4 * a + 3))) for a in range(3)]
    usable_ = torch.ones(n, do, ho, wo, dtype=torch.bool, device=dev)
    for sa in s:
        usable_ = usable_ & (sa.abs() <= MAX_COORD)            # false for a NaN too
    sizes = (di, hi, wi)
    zero, zero64 = torch.zeros((), dtype=dtype, device=dev), torch.zeros((), dtype=torch.float64, device=dev)

    def linear(idx):
        return ((idx[0].clamp(0, di - 1) * hi + idx[1].clamp(0, hi - 1)) * wi + idx[2].clamp(0, wi - 1)).reshape(n, -1)

    base, frac = [], []
    for sa in s:
        f = torch.where(usable_, sa.floor(), zero64)
        base.append(f.to(torch.int64))
        frac.append(torch.where(usable_, sa - f, zero64).to(dtype))
    acc = torch.zeros(n, do, ho, wo, dtype=dtype, device=dev)
    for c in range(8):
        k = (c >> 2, (c >> 1) & 1, c & 1)
        idx = [base[a] + k[a] for a in range(3)]
        inside = usable_
        for a in range(3):
            inside = inside & (idx[a] >= 0) & (idx[a] < sizes[a])
        w = [frac[a] if k[a] else 1 - frac[a] for a in range(3)]
        wgt = (w[0] * w[1]) * w[2]
        val = v.gather(1, linear(idx)).view(n, do, ho, wo)
        acc = acc + torch.where(inside, wgt * val, zero)
    out = acc * p32[:, 12].to(dtype).view(n, 1, 1, 1)
    out = out + p32[:, 13].to(dtype).view(n, 1, 1, 1)
    lead = image.shape[:image.dim() - 3]
    out = out.view(*lead, do, ho, wo)
    if lab is None:
        return out, None
    idx = [torch.where(usable_, (sa + 0.5).floor(), -torch.ones((), dtype=torch.float64, device=dev)).to(torch.int64) for sa in s]
    inside = usable_
    for a in range(3):
        inside = inside & (idx[a] >= 0) & (idx[a] < sizes[a])
    got = lab.reshape(n, -1).gather(1, linear(idx)).view(n, do, ho, wo)
    got = torch.where(inside, got, torch.zeros((), dtype=lab.dtype, device=dev))
    return out, got.view(*labels.shape[:labels.dim() - 3], do, ho, wo)


# ---- the table of a chain ------------------------------------------------------------------------------------------------------
def _cos_sin_deg(a):
    """cos and sin of an angle in degrees, exact (0, +-1) at the multiples of 90."""
    q = math.fmod(float(a), 360.0)
    if q % 90.0 == 0.0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q // 90) % 4]
    r = math.radians(q)
    return math.cos(r), math.sin(r)


def _rotation(angles):
    """Rx Ry Rz on (D, H, W): Rx turns the (H, W) plane, Ry the (D, W) plane, Rz the (D, H) plane; angles in degrees; fp64."""
    (cx, sx), (cy, sy), (cz, sz) = (_cos_sin_deg(a) for a in angles)
    rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return rx @ ry @ rz


def _per_sample(x, n, width, default, what):
    if x is None:
        x = default
    t = torch.as_tensor(x, dtype=torch.float64)
    t = t.expand(n, width) if width else t.expand(n)
    if t.shape != ((n, width) if width else (n,)):
        raise ValueError("%s: one value per sample%s" % (what, " and axis" if width else ""))
    return t


def compose_params(n, in_shape, angles=None, zoom=None, translate=None, flips=None, crop=None, gain=None, offset=None, shear=None):
    """The table (n, 16) fp32 (a CPU tensor) of the chain  rotate -> zoom -> translate -> [shear ->] flip -> crop  and of
    v * gain + offset, computed in fp64 and rounded once.  Per sample (a value without a batch axis is shared): angles (3) in
    DEGREES about (D, H, W), zoom (1), translate (3) in voxels, flips (3) booleans, crop (3) the integer offset of the output
    window, gain, offset, and shear (6) the coefficients (s01, s02, s10, s12, s20, s21) of Sh = I + those off-diagonal entries.

    With S = in_shape, c = (S - 1) / 2, R = Rx Ry Rz, F = diag(-1 where flipped), f = S - 1 where flipped else 0: the output ->
    source map is the product of the steps' maps in reverse chain order,
        src = c + (R / z) (F (o + crop) + f - tr - c),     i.e.  M = (R / z) F,  t = c + (R / z) (F crop + f - tr - c),
    and with a shear
        src = c + (R / z) (Sh (F (o + crop) + f - c) - tr),  i.e.  M = (R / z) Sh F,  t = c + (R / z) (Sh (F crop + f - c) - tr).
    shear=None is the first form, bit for bit.  The order of the six coefficients is MONAI's create_shear as remembered; it
    cannot be checked here (MONAI is not installed)."""
    size = torch.tensor([float(s) for s in in_shape], dtype=torch.float64)
    if size.shape != (3,):
        raise ValueError("in_shape: three extents")
    c = (size - 1) / 2
    angles = _per_sample(angles, n, 3, 0.0, "angles")
    zoom = _per_sample(zoom, n, 0, 1.0, "zoom")
    translate = _per_sample(translate, n, 3, 0.0, "translate")
    flips = _per_sample(None if flips is None else torch.as_tensor(flips).to(torch.float64), n, 3, 0.0, "flips")
    crop = _per_sample(crop, n, 3, 0.0, "crop")
    gain = _per_sample(gain, n, 0, 1.0, "gain")
    offset = _per_sample(offset, n, 0, 0.0, "offset")
    if shear is not None:
        shear = _per_sample(shear, n, 6, 0.0, "shear")
    if bool((zoom <= 0).any()):
        raise ValueError("zoom must be positive")
    table = torch.zeros(n, PARAMS, dtype=torch.float64)
    for i in range(n):
        a = _rotation(angles[i].tolist()) / zoom[i]
        sign = 1 - 2 * flips[i]
        if shear is None:
            m = a * sign[None, :]
            t = c + a @ (sign * crop[i] + flips[i] * (size - 1) - translate[i] - c)
        else:
            s01, s02, s10, s12, s20, s21 = shear[i].tolist()
            sh = torch.tensor([[1, s01, s02], [s10, 1, s12], [s20, s21, 1]], dtype=torch.float64)
            m = (a @ sh) * sign[None, :]
            t = c + a @ (sh @ (sign * crop[i] + flips[i] * (size - 1) - c) - translate[i])
        table[i, :12] = torch.cat((m, t[:, None]), 1).reshape(12)
        table[i, 12], table[i, 13] = gain[i], offset[i]
    return table.to(torch.float32)


# ---- the intensity tail: noise -> smooth -> gain -> offset -> contrast (include/transoar_augment.h) -------------------------------
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_MASK32 = 0xFFFFFFFF


def _mulhilo(m, x):
    """(hi, lo) 32-bit words of m * x for a constant m < 2^32 and an int64 tensor x of values < 2^32, without leaving int64:
    x is split into 16-bit halves, so every product stays below 2^48."""
    p, q = m * (x & 0xFFFF), m * (x >> 16)
    return (q + (p >> 16)) >> 16, (((q & 0xFFFF) << 16) + (p & _MASK32)) & _MASK32


def philox4x32(counter, key):
    """Philox4x32-10 in int64 arithmetic.  counter: four int64 tensors (or ints) of 32-bit words, key: two -> four int64 tensors."""
    c = [torch.as_tensor(x, dtype=torch.int64) & _MASK32 for x in counter]
    k = [torch.as_tensor(x, dtype=torch.int64) & _MASK32 for x in key]
    for _ in range(10):
        hi0, lo0 = _mulhilo(_PHILOX_M[0], c[0])
        hi1, lo1 = _mulhilo(_PHILOX_M[1], c[2])
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + _PHILOX_W[0]) & _MASK32, (k[1] + _PHILOX_W[1]) & _MASK32]
    return c


def philox_normals(count, k0, k1, dtype=torch.float64, device=None):
    """The normals of the voxels 0 .. count - 1 of samples with the keys k0, k1 (int64 tensors (n,)) -> (n, count) in `dtype`:
    voxel i takes word i & 3 of call i >> 2 (Box-Muller on the four words, see the header)."""
    calls = (count + 3) // 4
    j = torch.arange(calls, dtype=torch.int64, device=device)[None, :]
    k0 = torch.as_tensor(k0, dtype=torch.int64, device=device).view(-1, 1)
    k1 = torch.as_tensor(k1, dtype=torch.int64, device=device).view(-1, 1)
    zero = torch.zeros_like(j)
    r = philox4x32((j & _MASK32, j >> 32, zero, zero), (k0, k1))
    z = []
    for p in range(2):
        u1 = (((r[2 * p] >> 9).to(torch.float32) + 0.5) * 2.0 ** -23).to(dtype)      # exact in fp32
        u2 = ((r[2 * p + 1] >> 9).to(torch.float32) * 2.0 ** -23).to(dtype)
        rad = torch.sqrt(-2 * torch.log(u1))
        z += [rad * torch.cos(2 * math.pi * u2), rad * torch.sin(2 * math.pi * u2)]
    return torch.stack(z, -1).reshape(k0.shape[0], 4 * calls)[:, :count]


def smooth_tail(sigma):
    """The radius of MONAI's GaussianFilter(truncated=4) for a sigma, int(max(4 sigma, 0.5) + 0.5), in fp32 as the kernel."""
    s = torch.tensor(float(sigma), dtype=torch.float32)
    return int(torch.clamp(4 * s, min=0.5) + 0.5)


def smooth_weights(sigma, dtype=torch.float64, device=None):
    """The normalised taps x = -tail .. tail of MONAI's GaussianFilter(approx='erf', truncated=4) for an fp32 sigma in (0, 4]."""
    tail = smooth_tail(sigma)
    x = torch.arange(-tail, tail + 1, dtype=dtype, device=device)
    t = 0.70710678 / torch.tensor(_f32(sigma), dtype=dtype, device=device)
    w = (0.5 * (torch.erf(t * (x + 0.5)) - torch.erf(t * (x - 0.5)))).clamp(min=0)
    return w / w.sum()


def _tail_table(table, n):
    if not torch.is_tensor(table) or table.shape != (n, TAIL_WORDS) or table.dtype != torch.int32:
        raise ValueError("table: an int32 tensor of shape (%d, %d) (compose_intensity)" % (n, TAIL_WORDS))
    return table


def compose_intensity(n, flags=0, noise_mean=0.0, noise_std=0.0, sigma=(1.0, 1.0, 1.0), gain=1.0, offset=0.0, gamma=1.0, keys=(0, 0)):
    """The tail's table (n, 12) of 32-bit words, an int32 CPU tensor whose floating entries are fp32 bit patterns.  Per sample (a
    value without a batch axis is shared): flags (NOISE | SMOOTH | CONTRAST), noise_mean, noise_std, sigma (3) about (D, H, W),
    gain, offset, gamma, keys (2) of 32 bits each (given as non-negative integers)."""
    f = torch.zeros(n, TAIL_WORDS, dtype=torch.float32)
    f[:, 1] = _per_sample(noise_mean, n, 0, 0.0, "noise_mean")
    f[:, 2] = _per_sample(noise_std, n, 0, 0.0, "noise_std")
    f[:, 3:6] = _per_sample(sigma, n, 3, 1.0, "sigma")
    f[:, 6] = _per_sample(gain, n, 0, 1.0, "gain")
    f[:, 7] = _per_sample(offset, n, 0, 0.0, "offset")
    f[:, 8] = _per_sample(gamma, n, 0, 1.0, "gamma")
    table = f.view(torch.int32).clone()
    words = torch.cat((torch.as_tensor(flags, dtype=torch.int64).expand(n)[:, None], torch.as_tensor(keys, dtype=torch.int64).expand(n, 2)), 1)
    if bool(((words < 0) | (words > _MASK32)).any()):
        raise ValueError("flags and keys: 32-bit words, 0 .. 2^32 - 1")
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)              # the same bits
    table[:, 0], table[:, 9], table[:, 10] = words[:, 0], words[:, 1], words[:, 2]
    return table


def intensity_torch(image, table, dtype=torch.float32):
    """The specification of transoar_augment_intensity in torch on the inputs' device (index arithmetic and F.conv3d only; Philox
    in int64): image (N, [1,] D, H, W), table (N, 12) int32 -> the image in `dtype`, in the rank of the input.  Every flag of a
    row counts (there is no `steps`).  The path for CPU tensors and TRANSOAR_AUGMENT_HIP=0; with torch.float64 the tests'
    reference."""
    import torch.nn.functional as F
    img = _volume(image, "image")
    n, d, h, w = img.shape
    dev = img.device
    words = _tail_table(table, n).to(dev)
    f = words.view(torch.float32)
    flags = words[:, 0].to(torch.int64) & 7
    v = img.to(dtype)
    # noise
    on = ((flags & NOISE) != 0) & torch.isfinite(f[:, 1]) & torch.isfinite(f[:, 2])
    if bool(on.any()):
        z = philox_normals(d * h * w, words[:, 9].to(torch.int64) & _MASK32, words[:, 10].to(torch.int64) & _MASK32, dtype, dev)
        mean = torch.where(on, f[:, 1], torch.zeros_like(f[:, 1])).to(dtype).view(n, 1)
        std = torch.where(on, f[:, 2], torch.zeros_like(f[:, 2])).to(dtype).view(n, 1)
        v = torch.where(on.view(n, 1, 1, 1), v + (mean + std * z).view(n, d, h, w), v)
    # smoothing: a sample's three axes one after another, zero padding
    sig = f[:, 3:6]
    on = ((flags & SMOOTH) != 0) & ((sig > 0) & (sig <= MAX_SIGMA)).all(1)
    if bool(on.any()):
        rows = []
        for i in range(n):
            x = v[i][None, None]
            if bool(on[i]):
                for axis in range(3):
                    wts = smooth_weights(float(sig[i, axis]), dtype, dev)
                    shape, pad = [1, 1, 1, 1, 1], [0, 0, 0]
                    shape[2 + axis], pad[axis] = wts.numel(), wts.numel() // 2
                    x = F.conv3d(x, wts.view(shape), padding=pad)
            rows.append(x[0, 0])
        v = torch.stack(rows)
    # gain and offset (two roundings)
    gain = torch.where(torch.isfinite(f[:, 6]), f[:, 6], torch.ones_like(f[:, 6])).to(dtype).view(n, 1, 1, 1)
    offset = torch.where(torch.isfinite(f[:, 7]), f[:, 7], torch.zeros_like(f[:, 7])).to(dtype).view(n, 1, 1, 1)
    v = v * gain
    v = v + offset
    # contrast
    on = ((flags & CONTRAST) != 0) & torch.isfinite(f[:, 8]) & (f[:, 8] > 0)
    if bool(on.any()):
        mn = v.reshape(n, -1).min(1).values.view(n, 1, 1, 1)
        rng = v.reshape(n, -1).max(1).values.view(n, 1, 1, 1) - mn
        gamma = torch.where(on, f[:, 8], torch.ones_like(f[:, 8])).to(dtype).view(n, 1, 1, 1)
        y = ((v - mn) / (rng + 1e-7)) ** gamma * rng + mn
        v = torch.where(on.view(n, 1, 1, 1), y, v)
    return v.view(image.shape)


def intensity_workspace(n, device):
    """The device workspace of the kernel call for n samples (initialised by every call itself)."""
    return torch.empty(lib.transoar_augment_intensity_workspace_bytes(int(n)) // 4, dtype=torch.int32, device=device)


def intensity_into(image, image_out, table, steps, scratch=None, workspace=None):
    """The kernel sequence on the current stream: image (N, [1,] D, H, W) fp32 -> image_out (the same shape; may be `image`),
    table a DEVICE table (N, 12) int32, steps the union of the flags the table may carry, scratch a device tensor of the image's
    size (needed with SMOOTH in steps) and workspace from intensity_workspace; both are allocated here when not given (do give
    them under capture).  Capturable; nothing is read back."""
    img, out = _volume(image, "image"), _volume(image_out, "image_out")
    assert usable(img), "intensity_into: an fp32 CUDA image"
    assert img.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.shape == img.shape and out.device == img.device
    n, d, h, w = img.shape
    _tail_table(table, n)
    assert table.is_cuda and table.is_contiguous()
    steps = int(steps) & (NOISE | SMOOTH | CONTRAST)
    if steps & SMOOTH:
        if scratch is None:
            scratch = torch.empty_like(img)
        assert scratch.is_cuda and scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= img.numel()
        assert scratch.data_ptr() not in (img.data_ptr(), out.data_ptr())
    if workspace is None:
        workspace = intensity_workspace(n, img.device)
    assert workspace.is_cuda and workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= \
        lib.transoar_augment_intensity_workspace_bytes(n)
    _native.launch(lib.transoar_augment_intensity, img, img.data_ptr(), out.data_ptr(), _native.ptr(scratch) if steps & SMOOTH else None,
                   n, d, h, w, table.data_ptr(), steps, workspace.data_ptr())
    return image_out


# ---- the reference's configuration -> tables -------------------------------------------------------------------------------------
def upload_through_ring(rings, count, table, device):
    """A host table of any dtype -> (the table on `device`, copied from a pinned slot without blocking; the slot's event, to be
    recorded after the launch that reads the table).  `rings` is the caller's dict of rings, one per (device, rows) with `count`
    slots each; a slot is reused only after its event has completed (waited on when the ring wraps)."""
    key = (device, table.shape[0])
    ring = rings.get(key)
    if ring is None:
        ring = rings[key] = dict(next=0, slots=[
            dict(pinned=torch.empty(table.shape, dtype=table.dtype).pin_memory(),
                 device=torch.empty(table.shape, dtype=table.dtype, device=device), event=None)
            for _ in range(count)])
    slot = ring["slots"][ring["next"] % count]
    ring["next"] += 1
    if slot["event"] is None:
        slot["event"] = torch.cuda.Event()
    else:
        slot["event"].synchronize()          # the copy and the launch that read this slot `count` calls ago have finished
    slot["pinned"].copy_(table)
    slot["device"].copy_(slot["pinned"], non_blocking=True)
    return slot["device"], slot["event"]


class BatchAugment:
    """The reference's per-batch transform chain for `split` ('train', 'val' or 'test'), read from the reference's keys:
    config['augmentation'], config['foreground_voxel_statistics'] (percentile_00_5 / percentile_99_5 -> a_min / a_max),
    config['shape_statistics']['median'] (the translation range and, without a patch_size, the output shape).

    aug = BatchAugment(config, 'train', seed)
    x, lab = aug(image, labels)                       # (N, 1, Do, Ho, Wo) fp32 and labels: what TrainStep and Validator.add take
    aug(image, labels, out=step.static_inputs())      # straight into the captured step's buffers

    'val' and 'test' scale the range and crop only: centred with deterministic=True, at a random position otherwise (as the
    reference's RandSpatialCropd).  Cases whose stored shape is not the median go through transoar_amd.resize.TestSplit, which
    resizes them first as the reference's 'test' chain does.  On CUDA inputs a call draws on the host, copies the table from a pinned slot without blocking
    and launches: no host synchronisation per batch.  The pinned slots form a ring with one event each (recorded after the launch
    that reads the slot's table), waited on only when the ring wraps, so a draw never overwrites memory an earlier copy or launch
    may still be reading.

    full_chain=True ('train' only; 'val' and 'test' are unaffected) also takes p_shear, p_gaussian_noise, p_gaussian_smooth and
    p_adjust_contrast above 0.  Their parameters come from a SECOND generator seeded from `seed`, so the draws of the other steps
    and the spatial table are those of full_chain=False for the same seed.  Shear goes into the affine table.  When one of the
    three intensity probabilities is above 0 the intensity tail runs after the resample, in the reference's order noise -> smooth
    -> gain -> offset -> contrast: the resample's table then carries gain 1 and offset 0 and the tail's table (N, 12) the drawn
    ones; it is uploaded through a pinned ring of its own, the scratch volume and the workspace are kept per (device, shape), and
    the tail works in place on the resample's output (`out=` included).  Otherwise no tail is launched."""

    SLOTS = 4

    def __init__(self, config, split="train", seed=0, deterministic=False, full_chain=False):
        if split not in ("train", "val", "test"):
            raise ValueError("Please use 'test', 'val', or 'train' as split arg.")
        a = config["augmentation"]
        self.full_chain = bool(full_chain) and split == "train"
        self.tail_steps = 0
        if split == "train" and not self.full_chain:
            for key in UNSUPPORTED:
                if float(a.get(key, 0) or 0) > 0:
                    raise ValueError("augmentation.%s = %r: not part of the default device chain (only 0 is supported); "
                                     "BatchAugment(..., full_chain=True) implements it" % (key, a[key]))
        if self.full_chain:
            self._read_full_chain(a)
        self.split, self.deterministic, self.aug = split, bool(deterministic), a
        stats = config["foreground_voxel_statistics"]
        self.a_min, self.a_max = _f32(stats["percentile_00_5"]), _f32(stats["percentile_99_5"])
        if not self.a_max > self.a_min:
            raise ValueError("foreground_voxel_statistics: percentile_99_5 must exceed percentile_00_5")
        median = [float(s) for s in config["shape_statistics"]["median"]]
        patch = a.get("patch_size")
        self.out_shape = tuple(int(round(s)) for s in (median if patch is None else patch))
        self.translate_range = [m * float(a.get("translate_precentage", 0)) / 100 for m in median]
        self.generator = torch.Generator().manual_seed(int(seed))
        self.generator2 = torch.Generator().manual_seed((int(seed) + 0x9E3779B97F4A7C15) % (2 ** 63))      # shear and the tail
        self._slots, self._tail_slots, self._buffers = {}, {}, {}

    def _read_full_chain(self, a):
        """The ranges of the four opt-in steps, refused by key name where the kernels (or MONAI) would not take them."""
        on = lambda key: float(a.get(key, 0) or 0) > 0
        self.tail_steps = (NOISE if on("p_gaussian_noise") else 0) | (SMOOTH if on("p_gaussian_smooth") else 0) | \
            (CONTRAST if on("p_adjust_contrast") else 0)
        self.noise_mean, self.noise_std = float(a.get("gaussian_noise_mean", 0.0)), float(a.get("gaussian_noise_std", 0.1))
        if not math.isfinite(self.noise_mean) or not math.isfinite(self.noise_std) or self.noise_std < 0:
            raise ValueError("augmentation.gaussian_noise_std = %r (mean %r): a finite mean and a finite std >= 0"
                             % (a.get("gaussian_noise_std"), a.get("gaussian_noise_mean")))
        self.sigma = tuple(float(x) for x in a.get("gaussian_smooth_sigma", (0.5, 1.0)))
        if len(self.sigma) != 2 or not 0 < self.sigma[0] <= self.sigma[1] <= MAX_SIGMA:
            raise ValueError("augmentation.gaussian_smooth_sigma = %r: a range (lo, hi) with 0 < lo <= hi <= %g (a radius of at most "
                             "16 voxels)" % (a.get("gaussian_smooth_sigma"), MAX_SIGMA))
        self.gamma = tuple(float(x) for x in a.get("adjust_contrast_gamma", (0.5, 4.5)))
        if len(self.gamma) != 2 or not 0 < self.gamma[0] <= self.gamma[1] < math.inf:
            raise ValueError("augmentation.adjust_contrast_gamma = %r: a range (lo, hi) with 0 < lo <= hi" % (a.get("adjust_contrast_gamma"),))
        shear = list(a.get("shear_range", ()) or ())
        if len(shear) > 6:
            raise ValueError("augmentation.shear_range = %r: at most six entries" % (a.get("shear_range"),))
        self.shear_range = []
        for entry in shear + [0.0] * (6 - len(shear)):                   # padded with zeros; f -> U(-f, f), (a, b) -> U(a, b)
            lo, hi = (float(entry[0]), float(entry[1])) if isinstance(entry, (list, tuple)) else (-abs(float(entry)), abs(float(entry)))
            if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
                raise ValueError("augmentation.shear_range = %r: finite entries f or pairs (a, b) with a <= b" % (a.get("shear_range"),))
            self.shear_range.append((lo, hi))

    def _uniform2(self, n, lo, hi, width=None):
        shape = (n,) if width is None else (n, width)
        return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, generator=self.generator2)

    def _applied2(self, n, key):
        return torch.rand(n, dtype=torch.float64, generator=self.generator2) < float(self.aug.get(key, 0) or 0)

    def _uniform(self, n, lo, hi, width=None):
        shape = (n,) if width is None else (n, width)
        return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, generator=self.generator)

    def _applied(self, n, key):
        """Which samples take the step, with the probability of config['augmentation'][key]."""
        p = float(self.aug.get(key, 0) or 0)
        return torch.rand(n, dtype=torch.float64, generator=self.generator) < p

    def sample(self, n, in_shape=None):
        """The drawn steps of n samples, as compose_params takes them (identity values where a step is not applied)."""
        in_shape = self.out_shape if in_shape is None else tuple(int(s) for s in in_shape)
        if any(o > s for o, s in zip(self.out_shape, in_shape)):
            raise ValueError("the patch %s does not fit the stored volume %s" % (self.out_shape, in_shape))
        room = torch.tensor([s - o for s, o in zip(in_shape, self.out_shape)], dtype=torch.float64)
        steps = dict(angles=torch.zeros(n, 3, dtype=torch.float64), zoom=torch.ones(n, dtype=torch.float64),
                     translate=torch.zeros(n, 3, dtype=torch.float64), flips=torch.zeros(n, 3, dtype=torch.bool),
                     gain=torch.ones(n, dtype=torch.float64), offset=torch.zeros(n, dtype=torch.float64))
        if self.split == "train":
            a = self.aug
            lo, hi = (float(x) for x in a.get("rotation", (0, 0)))
            on = self._applied(n, "p_rotate")
            steps["angles"] = torch.where(on[:, None], self._uniform(n, lo, hi, 3), steps["angles"])
            on = self._applied(n, "p_zoom")
            steps["zoom"] = torch.where(on, self._uniform(n, float(a.get("min_zoom", 1)), float(a.get("max_zoom", 1))), steps["zoom"])
            on = self._applied(n, "p_translate")
            reach = torch.tensor(self.translate_range, dtype=torch.float64)
            steps["translate"] = torch.where(on[:, None], (2 * self._uniform(n, 0.0, 1.0, 3) - 1) * reach, steps["translate"])
            axes = [int(x) for x in a.get("flip_axis", (0, 1, 2))]
            for axis in axes:                                  # one RandFlipd per listed axis, each with p_flip
                steps["flips"][:, axis] = self._applied(n, "p_flip")
            f = float(a.get("intensity_scale_factors", 0))
            on = self._applied(n, "p_intensity_scale")
            steps["gain"] = torch.where(on, 1 + self._uniform(n, -f, f), steps["gain"])
            o = float(a.get("intensity_shift_offsets", 0))
            on = self._applied(n, "p_intensity_shift")
            steps["offset"] = torch.where(on, self._uniform(n, -o, o), steps["offset"])
        if self.split != "train" and self.deterministic:
            steps["crop"] = (room // 2).expand(n, 3).clone()
        else:
            steps["crop"] = torch.floor(self._uniform(n, 0.0, 1.0, 3) * (room + 1)).clamp(max=room)
        if self.full_chain and float(self.aug.get("p_shear", 0) or 0) > 0:
            on = self._applied2(n, "p_shear")
            lo = torch.tensor([r[0] for r in self.shear_range], dtype=torch.float64)
            hi = torch.tensor([r[1] for r in self.shear_range], dtype=torch.float64)
            steps["shear"] = torch.where(on[:, None], lo + (hi - lo) * self._uniform2(n, 0.0, 1.0, 6), torch.zeros(n, 6, dtype=torch.float64))
        return steps

    def sample_intensity(self, n, gain=None, offset=None):
        """The drawn tail of n samples, as compose_intensity takes it (gain and offset are those of sample())."""
        flags = torch.zeros(n, dtype=torch.int64)
        on = self._applied2(n, "p_gaussian_noise")
        std = torch.where(on, self._uniform2(n, 0.0, self.noise_std), torch.zeros(n, dtype=torch.float64))
        flags |= on.to(torch.int64) * NOISE
        on = self._applied2(n, "p_gaussian_smooth")
        sigma = self._uniform2(n, self.sigma[0], self.sigma[1], 3)
        flags |= on.to(torch.int64) * SMOOTH
        on = self._applied2(n, "p_adjust_contrast")
        gamma = torch.where(on, self._uniform2(n, self.gamma[0], self.gamma[1]), torch.ones(n, dtype=torch.float64))
        flags |= on.to(torch.int64) * CONTRAST
        keys = torch.randint(0, 2 ** 32, (n, 2), dtype=torch.int64, generator=self.generator2)
        return dict(flags=flags, noise_mean=self.noise_mean, noise_std=std, sigma=sigma, gamma=gamma, keys=keys,
                    gain=1.0 if gain is None else gain, offset=0.0 if offset is None else offset)

    def draw_both(self, n, in_shape=None):
        """-> (the table (n, 16) fp32, the tail's table (n, 12) int32 or None when no tail runs) of n freshly drawn samples."""
        in_shape = self.out_shape if in_shape is None else tuple(int(s) for s in in_shape)
        steps = self.sample(n, in_shape)
        tail = None
        if self.tail_steps:
            tail = compose_intensity(n, **self.sample_intensity(n, steps["gain"], steps["offset"]))
            steps["gain"], steps["offset"] = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        return check_table(compose_params(n, in_shape, **steps)), tail

    def draw(self, n, in_shape=None):
        """-> the table (n, 16) fp32 of n freshly drawn samples (a CPU tensor)."""
        return self.draw_both(n, in_shape)[0]

    def _tail_buffers(self, out):
        """The scratch volume and the workspace of the tail, kept per (device, shape)."""
        key = (out.device, tuple(out.shape))
        if key not in self._buffers:
            self._buffers[key] = (torch.empty_like(out) if self.tail_steps & SMOOTH else None, intensity_workspace(out.shape[0], out.device))
        return self._buffers[key]

    def _upload(self, table, device):
        """-> (the table on `device`, copied from a pinned slot of the ring without blocking; the slot's event, to be recorded
        after the launch that reads the table: it then covers both the copy out of the pinned slot and the kernel's reads)."""
        return upload_through_ring(self._slots, self.SLOTS, table, device)

    def __call__(self, image, labels=None, out=None):
        img = _volume(image, "image")
        n = img.shape[0]
        lab = None if labels is None else _volume(labels, "labels")
        (table, tail), event, tail_event = self.draw_both(n, img.shape[1:]), None, None
        if usable(img, lab):
            with torch.cuda.device(img.device):
                table, event = self._upload(table, img.device)
                if tail is not None:
                    tail, tail_event = upload_through_ring(self._tail_slots, self.SLOTS, tail, img.device)
        got = augment(img[:, None], None if lab is None else lab[:, None], table, self.out_shape, self.a_min, self.a_max, out=out)
        if event is not None:
            event.record(torch.cuda.current_stream(img.device))
        if tail is not None:
            x = got[0]
            if tail_event is not None:
                with torch.cuda.device(img.device):
                    scratch, workspace = self._tail_buffers(_volume(x, "image"))
                    intensity_into(x, x, tail, self.tail_steps, scratch, workspace)
                    tail_event.record(torch.cuda.current_stream(img.device))
            else:
                x.copy_(intensity_torch(x, tail.to(x.device)))
                if tail_event is not None:
                    tail_event.record(torch.cuda.current_stream(img.device))
        return got
