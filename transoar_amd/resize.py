"""Case resizing on the device (include/transoar_resize.h, csrc/resize.hip): the one step of the reference's data path that had no
counterpart here -- Resized(mode=['area', 'nearest']), behind CropForegroundd in the dataset preparation
(transoar/data/transforms.py:37-75, transform_preprocessing_amos / _visceral) and behind ScaleIntensityRanged in the 'test' chain
of get_transforms -- as ONE launch: an adaptive-average ("area") resize of the image and torch's fp32 nearest rule for the label
map, both read through a per-sample crop window and written as a crop of the resized grid.  The window of a case's foreground is
found on the device (two launches) and never leaves it, so crop-then-resize is capturable like the steps around it.

The window table (N, 12) int32 and the operation are specified in include/transoar_resize.h.  `resize_torch` and
`foreground_window_torch` are that specification in torch with explicit index arithmetic: the path for CPU tensors, for inputs
the kernels do not take and for TRANSOAR_RESIZE_HIP=0, and with dtype=torch.float64 the reference of the GPU tests.  a_min and
a_max are rounded to fp32 first in every path: the C ABI takes them as floats.

Two things rest on reading MONAI 0.7 from memory (MONAI is not installed where this was written): that Resized is
F.interpolate(mode=...) on the whole array, and CropForegroundd's clipped margin rule (see the header).

Out of scope: reading NIfTI files, orientation (Orientationd), the data_info.json statistics (foreground percentiles, the median
shape), and any tester or predictor class -- evaluation.Validator already has per_class, complete_only and predictions().
"""
import os

import torch

from . import _native
from .augment import _f32, _volume, upload_through_ring

lib = _native.bind("resize", abi=1)
ENABLED = os.environ.get("TRANSOAR_RESIZE_HIP", "1") != "0"
WINDOW = 12
MAX_EXTENT = 2 ** 24
_LABEL_DT = {torch.uint8: 16, torch.int16: 17, torch.int32: 18, torch.int64: 19}
_IMAGE_DT = {torch.float32: 0, torch.int16: 17}
AMOS_CLASSES = (1, 6, 7, 14, 15)          # crop_labels of transoar/data/transforms.py:29-32
AMOS_MARGIN = 2                           # transform_preprocessing_amos hard-codes margin=[2, 2, 2]


def _shape3(shape, what):
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or any(s < 1 for s in shape):
        raise ValueError("%s %s: three positive extents" % (what, shape))
    return shape


def _shapes(img, lab, resized_shape, out_shape):
    resized = _shape3(resized_shape, "resized_shape")
    out = resized if out_shape is None else _shape3(out_shape, "out_shape")
    if any(o > r for o, r in zip(out, resized)):
        raise ValueError("out_shape %s does not fit the resized grid %s" % (out, resized))
    if lab is not None and lab.shape != img.shape:
        raise ValueError("labels of shape %s for an image of shape %s" % (tuple(lab.shape), tuple(img.shape)))
    return resized, out


def _range(a_min, a_max):
    if (a_min is None) != (a_max is None):
        raise ValueError("a_min and a_max come together")
    if a_min is None:
        return None
    lo, hi = _f32(a_min), _f32(a_max)
    if not hi > lo:
        raise ValueError("a_max must exceed a_min")
    return lo, hi


def whole_window(n, shape):
    """The table of n whole volumes (a CPU tensor): start 0, extent = shape, crop 0, found 1."""
    row = torch.zeros(WINDOW, dtype=torch.int32)
    row[3:6] = torch.tensor(shape, dtype=torch.int32)
    row[9] = 1
    return row.expand(n, WINDOW).clone()


def check_window(window, shape, resized_shape, out_shape=None):
    """Refuse a HOST table the kernel would have to clamp: a start outside [0, S - 1], an extent outside [1, S - start] or a crop
    outside [0, R - out].  (A device table is not read back; the kernel clamps it.)"""
    resized, out = _shapes(None, None, resized_shape, out_shape)
    w = torch.as_tensor(window)
    if w.dim() != 2 or w.shape[1] != WINDOW or w.dtype not in (torch.int32, torch.int64):
        raise ValueError("window: an integer table of shape (N, %d)" % WINDOW)
    w = w.long()
    size = torch.tensor([int(s) for s in shape])
    room = torch.tensor([r - o for r, o in zip(resized, out)])
    start, extent, crop = w[:, 0:3], w[:, 3:6], w[:, 6:9]
    if bool((start < 0).any()) or bool((start > size - 1).any()):
        raise ValueError("window: a start outside the volume %s" % (tuple(size.tolist()),))
    if bool((extent < 1).any()) or bool((start + extent > size).any()):
        raise ValueError("window: an extent that is empty or leaves the volume %s" % (tuple(size.tolist()),))
    if bool((crop < 0).any()) or bool((crop > room).any()):
        raise ValueError("window: a crop outside [0, resized - out] = [0, %s]" % (tuple(room.tolist()),))
    return window


def usable(image, labels=None):
    """Can the kernels take these inputs?  (labels alone: usable(None, labels), for foreground_window)"""
    ok = ENABLED
    if ok and image is not None:
        ok = (torch.is_tensor(image) and image.is_cuda and image.dtype in _IMAGE_DT and image.dim() in (4, 5)
              and image.numel() > 0 and image.shape[0] <= 65535)
    if ok and labels is not None:
        ok = (torch.is_tensor(labels) and labels.is_cuda and labels.dtype in _LABEL_DT and labels.dim() in (4, 5)
              and labels.numel() > 0 and labels.shape[0] <= 65535 and (image is None or labels.device == image.device))
    return bool(ok and (image is not None or labels is not None))


# ---- the specification in torch --------------------------------------------------------------------------------------------------
def _clamped_rows(window, n, shape, resized, out):
    """The table as the kernel uses it: python ints per sample, clamped (start, extent, crop)."""
    if window is None:
        return [((0, 0, 0), tuple(shape), (0, 0, 0))] * n
    w = torch.as_tensor(window).detach().cpu().long()
    if w.shape != (n, WINDOW):
        raise ValueError("window: a table of shape (%d, %d), got %s" % (n, WINDOW, tuple(w.shape)))
    rows = []
    for r in w.tolist():
        start = [min(max(r[a], 0), shape[a] - 1) for a in range(3)]
        extent = [min(max(r[3 + a], 1), shape[a] - start[a]) for a in range(3)]
        crop = [min(max(r[6 + a], 0), resized[a] - out[a]) for a in range(3)]
        rows.append((tuple(start), tuple(extent), tuple(crop)))
    return rows


def nearest_index(o, extent, resized):
    """torch's nearest source index of the resized indices `o` (an integer tensor): fp32 arithmetic, as upsample_nearest3d."""
    scale = torch.tensor(float(extent), dtype=torch.float32) / torch.tensor(float(resized), dtype=torch.float32)
    return (o.to(torch.float32) * scale).floor().to(torch.int64).clamp(max=extent - 1)


def _area_axis(v, axis, o, start, extent, resized):
    """Sum `v` over the bins of the resized indices `o` along `axis`: -> (sums, counts)."""
    lo = (o * extent) // resized
    hi = -((-(o + 1) * extent) // resized)
    count = hi - lo
    k = int(count.max())
    step = torch.arange(k, device=o.device)
    idx = (lo[:, None] + step[None, :]).clamp(max=extent - 1) + start
    inside = step[None, :] < count[:, None]
    picked = v.index_select(axis, idx.reshape(-1))
    shape = list(v.shape)
    shape[axis:axis + 1] = [o.numel(), k]
    picked = picked.reshape(shape)
    mask_shape = [1] * len(shape)
    mask_shape[axis], mask_shape[axis + 1] = o.numel(), k
    picked = torch.where(inside.reshape(mask_shape), picked, torch.zeros((), dtype=v.dtype, device=v.device))
    return picked.sum(axis + 1), count


def resize_torch(image, labels, window, resized_shape, out_shape=None, a_min=None, a_max=None, dtype=torch.float32):
    """The specification of include/transoar_resize.h in torch on the inputs' device, one sample at a time (the windows differ):
    the table is clamped as the kernel clamps it, the bins are exact integer arithmetic, the nearest rule is fp32.  The range
    scaling, the sums and the division are in `dtype` (the bins are summed W first, then H, then D); with torch.float64 it is the
    reference of the tests.  -> (image in `dtype`, labels of their own type or None), in the rank of the inputs."""
    img = _volume(image, "image")
    lab = None if labels is None else _volume(labels, "labels")
    resized, out = _shapes(img, lab, resized_shape, out_shape)
    n, shape, dev = img.shape[0], tuple(img.shape[1:]), img.device
    rng = _range(a_min, a_max)
    rows = _clamped_rows(window, n, shape, resized, out)
    got = torch.empty(n, *out, dtype=dtype, device=dev)
    got_lab = None if lab is None else torch.empty(n, *out, dtype=lab.dtype, device=dev)
    for s, (start, extent, crop) in enumerate(rows):
        v = img[s].to(dtype)
        if rng is not None:
            lo = torch.tensor(rng[0], dtype=dtype, device=dev)
            span = (torch.tensor(rng[1], dtype=torch.float32, device=dev) - lo.to(torch.float32)).to(dtype)      # the kernel's fp32 range
            v = ((v - lo) / span).clamp(0, 1)
        grid = [torch.arange(crop[a], crop[a] + out[a], device=dev) for a in range(3)]
        counts = []
        for a in (2, 1, 0):
            v, c = _area_axis(v, a, grid[a], start[a], extent[a], resized[a])
            counts.append(c)
        cw, ch, cd = counts
        count = cd[:, None, None] * ch[None, :, None] * cw[None, None, :]
        got[s] = v / count.to(torch.float32).to(dtype)
        if lab is not None:
            idx = [nearest_index(grid[a], extent[a], resized[a]) + start[a] for a in range(3)]
            got_lab[s] = lab[s][idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
    lead = image.shape[:image.dim() - 3]
    got = got.view(*lead, *out)
    return got, (None if lab is None else got_lab.view(*labels.shape[:labels.dim() - 3], *out))


def _class_mask(classes):
    if classes is None:
        return -1
    mask = 0
    for c in classes:
        c = int(c)
        if not 1 <= c <= 62:
            raise ValueError("classes: ids in 1..62, got %d" % c)
        mask |= 1 << c
    return mask


def _margins(margin):
    m = [int(margin)] * 3 if isinstance(margin, (int, float)) else [int(x) for x in margin]
    if len(m) != 3 or any(x < 0 or x > MAX_EXTENT for x in m):
        raise ValueError("margin: one or three values in 0..2^24, got %r" % (margin,))
    return m


def foreground_window_torch(labels, classes=None, margin=0):
    """The foreground window of include/transoar_resize.h in torch on the labels' device -> the table (N, 12) int32."""
    lab = _volume(labels, "labels")
    mask, m = _class_mask(classes), _margins(margin)
    n, shape, dev = lab.shape[0], tuple(lab.shape[1:]), lab.device
    if mask < 0:
        sel = lab > 0
    else:
        sel = torch.zeros_like(lab, dtype=torch.bool)
        for c in range(1, 63):
            if mask >> c & 1:
                sel |= lab == c
    table = torch.zeros(n, WINDOW, dtype=torch.int64, device=dev)
    found = sel.reshape(n, -1).any(1)
    for a in range(3):
        line = sel.to(torch.uint8).amax(dim=tuple(d for d in (1, 2, 3) if d != a + 1)).to(torch.int64)          # (n, S_a)
        lo = line.argmax(1)
        hi = shape[a] - 1 - line.flip(1).argmax(1)
        start = (lo - m[a]).clamp(min=0)
        end = (hi + 1 + m[a]).clamp(max=shape[a])
        table[:, a] = torch.where(found, start, torch.zeros_like(start))
        table[:, 3 + a] = torch.where(found, end - start, torch.full_like(start, shape[a]))
    table[:, 9] = found.to(torch.int64)
    return table.to(torch.int32)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def workspace_bytes(n, voxels_per_sample):
    return int(lib.transoar_foreground_window_workspace_bytes(int(n), int(voxels_per_sample)))


def foreground_window_into(labels, window, workspace, classes=None, margin=0):
    """The two launches on the current stream: labels (N, [1,] D, H, W) CUDA integers -> window (N, 12) int32 in place.
    workspace: an int32 CUDA tensor of at least workspace_bytes(N, D * H * W) bytes.  Capturable; nothing is read back."""
    lab = _volume(labels, "labels")
    assert usable(None, lab), "foreground_window_into: uint8 / int16 / int32 / int64 CUDA labels"
    assert lab.is_contiguous() and window.is_cuda and window.dtype == torch.int32 and window.is_contiguous()
    assert window.shape == (lab.shape[0], WINDOW) and workspace.is_cuda and workspace.is_contiguous()
    n, sd, sh, sw = lab.shape
    m = _margins(margin)
    _native.launch(lib.transoar_foreground_window, lab, lab.data_ptr(), _LABEL_DT[lab.dtype], n, sd, sh, sw, _class_mask(classes),
                   m[0], m[1], m[2], window.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size())
    return window


def foreground_window(labels, classes=None, margin=0, out=None):
    """-> the window table (N, 12) int32 on the labels' device: per sample the bounding window of the voxels whose label is in
    `classes` (an iterable of ids in 1..62; None: every label > 0), grown by `margin` (one value or three) and clipped to the
    volume; the whole volume and found = 0 where no voxel is selected.  CUDA labels go through the kernels (the table stays on
    the device), anything else through foreground_window_torch."""
    lab = _volume(labels, "labels")
    if not usable(None, lab):
        got = foreground_window_torch(lab, classes, margin)
        if out is not None:
            out.copy_(got)
            return out
        return got
    lab = lab.contiguous()
    n = lab.shape[0]
    if out is None:
        out = torch.empty(n, WINDOW, dtype=torch.int32, device=lab.device)
    ws = torch.empty(max(workspace_bytes(n, lab[0].numel()) // 4, 1), dtype=torch.int32, device=lab.device)
    return foreground_window_into(lab, out, ws, classes, margin)


def resize_into(image, labels, window, resized_shape, image_out, labels_out, a_min=None, a_max=None):
    """The kernel on the current stream: image (N, [1,] D, H, W) fp32 or int16, labels the same shape or None, window a DEVICE
    table (N, 12) int32 or None -> image_out (N, [1,] Do, Ho, Wo) fp32 and labels_out in place.  Capturable; nothing is read
    back."""
    img, out = _volume(image, "image"), _volume(image_out, "image_out")
    lab = None if labels is None else _volume(labels, "labels")
    lout = None if labels_out is None else _volume(labels_out, "labels_out")
    resized, _ = _shapes(img, lab, resized_shape, out.shape[1:])
    rng = _range(a_min, a_max)
    assert usable(img, lab), "resize_into: fp32 / int16 CUDA image (and uint8 / int16 / int32 / int64 CUDA labels)"
    assert img.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == img.shape[0] and out.is_cuda
    assert (lab is None) == (lout is None)
    if lab is not None:
        assert lab.is_contiguous() and lout.is_contiguous() and lout.dtype == lab.dtype and lout.shape == out.shape and lout.is_cuda
    if window is not None:
        assert window.is_cuda and window.dtype == torch.int32 and window.is_contiguous() and window.shape == (img.shape[0], WINDOW)
    n, di, hi, wi = img.shape
    _native.launch(lib.transoar_resize_forward, img, img.data_ptr(), _IMAGE_DT[img.dtype], _native.ptr(lab),
                   _LABEL_DT[lab.dtype] if lab is not None else 0, n, di, hi, wi, resized[0], resized[1], resized[2],
                   out.shape[1], out.shape[2], out.shape[3], _native.ptr(window), 0 if rng is None else 1,
                   0.0 if rng is None else rng[0], 1.0 if rng is None else rng[1], out.data_ptr(), _native.ptr(lout))


def resize(image, labels, resized_shape, out_shape=None, window=None, a_min=None, a_max=None, out=None):
    """-> (image (N, [1,] Do, Ho, Wo) fp32, labels of their own type or None), in the rank of the inputs: the window of every
    sample resized to `resized_shape` (area for the image, nearest for the labels) and cropped to `out_shape` at the table's
    crop offsets.  window: None (the whole volume), a HOST table (checked by check_window and uploaded) or a device table (taken
    as it is; the kernel clamps it).  a_min / a_max: range scaling first.  out=(image_out, labels_out) writes in place.  CUDA
    inputs go through the kernel, anything else (and TRANSOAR_RESIZE_HIP=0) through resize_torch."""
    img = _volume(image, "image")
    lab = None if labels is None else _volume(labels, "labels")
    resized, out_shape = _shapes(img, lab, resized_shape, out_shape)
    if window is not None:
        if not torch.is_tensor(window) or window.shape != (img.shape[0], WINDOW):
            raise ValueError("window: a tensor of shape (%d, %d)" % (img.shape[0], WINDOW))
        if not window.is_cuda:
            check_window(window, img.shape[1:], resized, out_shape)
    if not usable(img, lab):
        got = resize_torch(image, labels, window, resized, out_shape, a_min, a_max)
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
    table = None if window is None else window.to(device=img.device, dtype=torch.int32, non_blocking=True).contiguous()
    resize_into(image.contiguous(), None if lab is None else labels.contiguous(), table, resized, out[0],
                None if lab is None else out[1], a_min, a_max)
    return out[0], (out[1] if lab is not None else None)


# ---- the reference's two callers -------------------------------------------------------------------------------------------------
class PrepareCase:
    """The reference's dataset preparation of one case after loading: CropForegroundd on the label map, then
    Resized(mode=['area', 'nearest']) to the fixed training shape (transform_preprocessing_amos / _visceral).

    prep = PrepareCase.from_config(preprocessing_config)        # or PrepareCase(resize_shape, classes, margin)
    image, labels, window = prep(raw_image, raw_labels)         # fp32 image and int32 labels of resize_shape: data.npy / label.npy

    raw_image: (N, [1,] D, H, W) fp32 or int16; raw_labels: the same shape, uint8 / int16 / int32 / int64.  Orientation
    (Orientationd) is the caller's business: the inputs are taken as stored.  On CUDA inputs the foreground window and the resize
    run back to back on the current stream with no host synchronisation between them; the window table (N, 12) int32 is returned
    on the inputs' device."""

    def __init__(self, resize_shape, classes=None, margin=0):
        self.resize_shape = _shape3(resize_shape, "resize_shape")
        self.classes = None if classes is None else tuple(sorted(int(c) for c in classes))
        _class_mask(self.classes)
        self.margin = tuple(_margins(margin))

    @classmethod
    def from_config(cls, preprocessing_config):
        """dataset_config 'amos': the organs and the margin transform_preprocessing_amos hard-codes ({1, 6, 7, 14, 15}, 2; the
        YAML's margin is not read there); 'visceral': every label > 0 and the YAML's margin."""
        name = preprocessing_config["dataset_config"]
        if name == "amos":
            return cls(preprocessing_config["resize_shape"], AMOS_CLASSES, AMOS_MARGIN)
        if name == "visceral":
            return cls(preprocessing_config["resize_shape"], None, preprocessing_config["margin"])
        raise ValueError("dataset_config %r: 'amos' or 'visceral'" % (name,))

    def __call__(self, image, labels):
        window = foreground_window(labels, self.classes, self.margin)
        got, got_lab = resize(image, labels, self.resize_shape, window=window)
        return got, got_lab.to(torch.int32), window


class TestSplit:
    """The reference's 'test' chain (get_transforms('test')): range scaling from config['foreground_voxel_statistics'], an area /
    nearest resize of every case to config['shape_statistics']['median'], then a crop of config['augmentation']['patch_size']
    (none without a patch_size) -- centred with deterministic=True, otherwise at a position drawn from this object's own seeded
    CPU generator (as the reference's RandSpatialCropd, not MONAI's stream).

    split = TestSplit(config, seed)
    x, lab = split(image, labels)            # (N, 1, Do, Ho, Wo) fp32 and labels: what Validator.add takes
    split(image, labels, out=(x, lab))       # in place

    On CUDA inputs the table goes up through a ring of pinned slots (augment.upload_through_ring, as BatchAugment): no host
    synchronisation per batch."""

    __test__ = False          # not a test class, whatever its name says to pytest
    SLOTS = 4

    def __init__(self, config, seed=0, deterministic=False):
        stats = config["foreground_voxel_statistics"]
        self.a_min, self.a_max = _f32(stats["percentile_00_5"]), _f32(stats["percentile_99_5"])
        if not self.a_max > self.a_min:
            raise ValueError("foreground_voxel_statistics: percentile_99_5 must exceed percentile_00_5")
        self.resized_shape = tuple(int(round(float(s))) for s in config["shape_statistics"]["median"])
        patch = config["augmentation"].get("patch_size")
        self.out_shape = self.resized_shape if patch is None else tuple(int(round(float(s))) for s in patch)
        if any(o > r for o, r in zip(self.out_shape, self.resized_shape)):
            raise ValueError("the patch %s does not fit the median shape %s" % (self.out_shape, self.resized_shape))
        self.deterministic = bool(deterministic)
        self.generator = torch.Generator().manual_seed(int(seed))
        self._slots = {}

    def draw(self, n, in_shape):
        """-> the window table (n, 12) int32 of n cases of the stored shape `in_shape` (a CPU tensor): the whole volume, and the
        crop offsets of the patch in the resized grid."""
        table = whole_window(n, _shape3(in_shape, "in_shape"))
        room = torch.tensor([r - o for r, o in zip(self.resized_shape, self.out_shape)], dtype=torch.float64)
        if self.deterministic:
            crop = (room // 2).expand(n, 3)
        else:
            u = torch.rand((n, 3), dtype=torch.float64, generator=self.generator)
            crop = torch.floor(u * (room + 1)).clamp(max=room)
        table[:, 6:9] = crop.to(torch.int32)
        return table

    def split(self, image, labels=None, out=None):
        img = _volume(image, "image")
        lab = None if labels is None else _volume(labels, "labels")
        table, event = self.draw(img.shape[0], img.shape[1:]), None
        if usable(img, lab):
            with torch.cuda.device(img.device):
                table, event = upload_through_ring(self._slots, self.SLOTS, table, img.device)
        got = resize(img[:, None], None if lab is None else lab[:, None], self.resized_shape, self.out_shape, window=table,
                     a_min=self.a_min, a_max=self.a_max, out=out)
        if event is not None:
            event.record(torch.cuda.current_stream(img.device))
        return got

    __call__ = split
