"""ctypes binding and autograd shim of the LDS-tiled implicit-GEMM convolution kernels (C ABI:
include/transoar_convgemm.h): the 3x3x3 convolutions of the encoder stages from 48 channels up and of the FPN `out`
layers (encoder_blocks.py:28-51, attn_fpn.py:65-73,126), forward, data gradient (stride 1: one launch with the
mirrored tap list; stride 2: the eight parity classes of the dx voxels in one launch -- up to 32 input channels the
halo-tile kernel that writes dx as whole lines) and weight gradient -- and the
weight gradient of a token projection as the one-tap case.  No fallback: the library must be built."""
import os

import torch

from . import _native
from . import conv_plan as _plan
from ._native import launch, ptr

ABI_VERSION = 3
CL3D = torch.channels_last_3d
lib = _native.bind("convgemm", abi=ABI_VERSION)
DGRAD_S2_HALO = _plan.KNOBS.dgrad_s2_halo          # read by tests; the switch itself lives in conv_plan.KNOBS


def _taps(entries):
    """[(delta, t), ...] -> packed per-axis tap list (include/transoar_convgemm.h)."""
    v = len(entries)
    for e, (delta, t) in enumerate(entries):
        v |= ((delta + 1) << (2 + 4 * e)) | (t << (4 + 4 * e))
    return v


TAPS_FWD = _taps([(-1, 0), (0, 1), (1, 2)])        # source = s*m + t - 1
TAPS_DGRAD1 = _taps([(1, 0), (0, 1), (-1, 2)])     # source = m + 1 - t
TAPS_PARITY = (_taps([(0, 1)]), _taps([(1, 0), (0, 2)]))     # dx voxel 2m + p: p = 0 sees tap 1 of dy m; p = 1 taps 0, 2 of dy m+1, m
TAPS_ONE = _taps([(0, 1)])


def pack_fwd(weight):
    """(Cout, Cin, 3,3,3) -> (27, Cout, Cin) bf16."""
    co, ci = weight.shape[:2]
    return weight.permute(2, 3, 4, 0, 1).reshape(27, co, ci).to(torch.bfloat16).contiguous()


def pack_dgrad(weight):
    """(Cout, Cin, 3,3,3) -> (27, Cin, Cout) bf16: the data gradient contracts over Cout."""
    co, ci = weight.shape[:2]
    return weight.permute(2, 3, 4, 1, 0).reshape(27, ci, co).to(torch.bfloat16).contiguous()


def pack_both(weight):
    """fp32 contiguous (Cout, Cin, 3,3,3) -> (wk (27, Cout, Cin), wkt (27, Cin, Cout)) bf16.  TRANSOAR_CONV_PACK_HIP=1: in one
    kernel (transoar_conv3d_pack) -- measured 0.5 ms per step SLOWER than torch's two permute-and-cast copies (its 32 x 32
    tiles are 2 to 576 blocks per layer: the small layers do not fill the chip), so it is off by default."""
    co, ci = weight.shape[:2]
    if weight.dtype != torch.float32 or not weight.is_contiguous() or not os.environ.get("TRANSOAR_CONV_PACK_HIP"):
        return pack_fwd(weight), pack_dgrad(weight)
    wk = torch.empty((27, co, ci), dtype=torch.bfloat16, device=weight.device)
    wkt = torch.empty((27, ci, co), dtype=torch.bfloat16, device=weight.device)
    launch(lib.transoar_conv3d_pack, weight, weight.data_ptr(), wk.data_ptr(), wkt.data_ptr(), co, ci)
    return wk, wkt


class PackPlan:
    """Both filter packs of MANY convolution layers in one launch (transoar_conv3d_pack_many), into persistent buffers.
    modules: objects with a contiguous fp32 `.weight` (Cout, Cin, 3,3,3); after run() each module carries
    `_packs = (wk, wkt)` and `_packs_version = weight._version`, which conv3d.Conv3dK3 uses as long as the weight has not
    been written since (an optimizer step bumps the version; a captured graph replays the pack kernel with the step)."""

    def __init__(self, modules):
        self.modules = list(modules)
        assert self.modules
        dev = self.modules[0].weight.device
        self.buffers, rows, tile = [], [], 0
        for m in self.modules:
            w = m.weight
            assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[2:]) == (3, 3, 3) and w.device == dev
            co, ci = w.shape[:2]
            wk = torch.empty((27, co, ci), dtype=torch.bfloat16, device=dev)
            wkt = torch.empty((27, ci, co), dtype=torch.bfloat16, device=dev)
            self.buffers.append((wk, wkt))
            rows.append([w.data_ptr(), wk.data_ptr(), wkt.data_ptr(), co | (ci << 32), tile])
            tile += ((co + 31) // 32) * ((ci + 31) // 32)
        self.total_tiles = tile
        self.ptrs = [r[0] for r in rows]
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)

    def valid(self):
        return all(m.weight.data_ptr() == p for m, p in zip(self.modules, self.ptrs))

    def run(self):
        launch(lib.transoar_conv3d_pack_many, self.table, self.table.data_ptr(), len(self.modules), self.total_tiles)
        for m, packs in zip(self.modules, self.buffers):
            m._packs, m._packs_version = packs, m.weight._version


def _igemm(x, wk, bias, out, src_dims, cin, cout, m_dims, src_stride, out_dims, out_stride, parity, taps, n, split, classes=0):
    """One launch of transoar_conv3d_igemm (+ the summing / cast pass when split > 1); `out` is the whole output map."""
    if split > 1:
        rows_out = n * out_dims[0] * out_dims[1] * out_dims[2]
        part = torch.empty((split, rows_out, cout), dtype=torch.float32, device=x.device)      # written completely
        launch(lib.transoar_conv3d_igemm, x, x.data_ptr(), wk.data_ptr(), None, None, part.data_ptr(), n, *src_dims, cin, cout,
               *m_dims, src_stride, *out_dims, out_stride, *parity, *taps, split, classes)
        launch(lib.transoar_conv3d_finish, x, part.data_ptr(), ptr(bias), out.data_ptr(), rows_out, cout, split)
    else:
        launch(lib.transoar_conv3d_igemm, x, x.data_ptr(), wk.data_ptr(), ptr(bias), out.data_ptr(), None, n, *src_dims, cin, cout,
               *m_dims, src_stride, *out_dims, out_stride, *parity, *taps, 1, classes)


def _batch(ranges, n, *tensors):
    """(count, split or chunks, the tensors' views of the batch range) of every range of a plan."""
    for i, c, k in ranges:
        yield (c, k) + (tensors if c == n else tuple(t[i:i + c] for t in tensors))


def conv_forward(x, wk, bias, stride, split=None, ranges=None):
    """x (N, Cin, D, H, W) NDHWC bf16, wk (27, Cout, Cin) bf16, bias fp32 or None -> (N, Cout, Do, Ho, Wo) NDHWC bf16.
    split: the split-K factor instead of the plan's; ranges: conv_plan.igemm_ranges of the shape, when the caller has them."""
    n, ci, d, h, w = x.shape
    co = wk.shape[1]
    od, oh, ow = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
    y = torch.empty((n, co, od, oh, ow), dtype=torch.bfloat16, device=x.device, memory_format=CL3D)
    for c, s, xs, ys in _batch(ranges or _plan.igemm_ranges(n, od * oh * ow, ci, co, 27, "conv_forward"), n, x, y):
        _igemm(xs, wk, bias, ys, (d, h, w), ci, co, (od, oh, ow), stride, (od, oh, ow), 1, (0, 0, 0), (TAPS_FWD,) * 3, c, split or s)
    return y


def dgrad_s2_halo(gy, wkt, in_dims):
    """Stride 2, few input channels: dx as whole lines, all eight parity classes of a tile in one workgroup."""
    n, co, od, oh, ow = gy.shape
    ci = wkt.shape[1]
    gx = torch.empty((n, ci) + tuple(in_dims), dtype=torch.bfloat16, device=gy.device, memory_format=CL3D)
    launch(lib.transoar_conv3d_dgrad_s2_halo, gy, gy.data_ptr(), wkt.data_ptr(), gx.data_ptr(), n, od, oh, ow, *in_dims, ci, co)
    return gx


def dgrad_igemm(gy, wkt, stride, in_dims, ranges, split=None):
    """The implicit-GEMM data gradient: stride 1 with the mirrored tap list; stride 2 the eight parity classes (pd, ph, pw)
    of the dx voxels in one launch."""
    n, co, od, oh, ow = gy.shape
    ci = wkt.shape[1]
    dims = tuple(in_dims)
    gx = torch.empty((n, ci) + dims, dtype=torch.bfloat16, device=gy.device, memory_format=CL3D)
    for c, s, gys, gxs in _batch(ranges, n, gy, gx):
        if stride == 1:
            _igemm(gys, wkt, None, gxs, (od, oh, ow), co, ci, dims, 1, dims, 1, (0, 0, 0), (TAPS_DGRAD1,) * 3, c, split or s)
        else:
            _igemm(gys, wkt, None, gxs, (od, oh, ow), co, ci, (1, 1, 1), 1, dims, 2, (0, 0, 0), (TAPS_ONE,) * 3, c, split or s, classes=1)
    return gx


def conv_dgrad(gy, wkt, stride, in_dims, split=None):
    """gy (N, Cout, Do, Ho, Wo) NDHWC bf16, wkt (27, Cin, Cout) bf16 -> dx (N, Cin, D, H, W) NDHWC bf16.
    split: that split-K factor on the implicit GEMM (stride 2: the parity-class launch, never the halo-tile kernel)."""
    route, ranges = _plan.dgrad_gemm(gy.shape[0], wkt.shape[1], gy.shape[1], *in_dims, stride, general=split is not None)
    if route == "s2_halo":
        return dgrad_s2_halo(gy, wkt, in_dims)
    return dgrad_igemm(gy, wkt, stride, in_dims, ranges, split)


def _wgrad(x2, gy2, geom, taps, taps_out, out_shape, chunks=None):
    n, sd, sh, sw, ci, co, md, mh, mw, stride = geom
    chunks = chunks or _plan.wgrad_chunks(n * md * mh * mw, ci, co, taps_out)
    part = torch.empty(lib.transoar_conv3d_wgrad_part_floats(ci, co, chunks, taps_out), dtype=torch.float32, device=x2.device)
    dw = torch.empty(out_shape, dtype=torch.float32, device=x2.device)
    launch(lib.transoar_conv3d_wgrad, x2, gy2.data_ptr(), x2.data_ptr(), part.data_ptr(), dw.data_ptr(), n, sd, sh, sw, ci, co,
           md, mh, mw, stride, *taps, chunks, taps_out)
    return dw


def conv_wgrad_ring(x, gy, stride, chunks=None):
    """The LDS-ring weight gradient (conv_wgrad_ring.hpp); conv_plan.wgrad_gemm says which layers take it."""
    n, ci, d, h, w = x.shape
    co, od, oh, ow = gy.shape[1:]
    chunks = chunks or _plan.WGRAD_RING_CHUNKS
    part = torch.empty(lib.transoar_conv3d_wgrad_part_floats(ci, co, chunks, 27), dtype=torch.float32, device=x.device)
    dw = torch.empty((co, ci, 3, 3, 3), dtype=torch.float32, device=x.device)
    launch(lib.transoar_conv3d_wgrad_ring, x, gy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), n, d, h, w, ci, co,
           od, oh, ow, stride, chunks)
    return dw


def wgrad_voxel_major(x, gy, stride, ranges):
    """The general voxel-major weight gradient, one launch per batch range: the filter gradient is a sum over samples."""
    n, ci, d, h, w = x.shape
    co, od, oh, ow = gy.shape[1:]
    dw = None
    for c, chunks, xs, gys in _batch(ranges, n, x, gy):
        part = _wgrad(xs, gys, (c, d, h, w, ci, co, od, oh, ow, stride), (TAPS_FWD,) * 3, 27, (co, ci, 3, 3, 3), chunks)
        dw = part if dw is None else dw.add_(part)
    return dw


def conv_wgrad(x, gy, stride):
    """x (N, Cin, D, H, W), gy (N, Cout, Do, Ho, Wo) NDHWC bf16 -> dW (Cout, Cin, 3, 3, 3) fp32."""
    route, detail = _plan.wgrad_gemm(x.shape[0], x.shape[1], *gy.shape[1:])
    return conv_wgrad_ring(x, gy, stride) if route == "ring" else wgrad_voxel_major(x, gy, stride, detail)


def linear_wgrad(x, gy):
    """x (T, K), gy (T, N) bf16 contiguous -> dW (N, K) fp32 = gy^T x (the one-tap case)."""
    t, k = x.shape
    nn_ = gy.shape[1]
    return _wgrad(x, gy, (1, 1, 1, t, k, nn_, 1, 1, t, 1), (TAPS_ONE,) * 3, 1, (nn_, k))


def linear_wgrad_bias_usable(k, n):
    """Does the last K tile have a padding column for the ones that sum gy (transoar_linear_wgrad_bias)?"""
    return k % (64 if (k <= 64 and n <= 64) else 128) != 0


def linear_wgrad_bias(x, gy):
    """x (T, K), gy (T, N) bf16 contiguous -> (dW (N, K), db (N,)) fp32 = (gy^T x, gy.sum(0)) in one pass over gy."""
    t, k = x.shape
    nn_ = gy.shape[1]
    chunks = _plan.wgrad_chunks(t, k, nn_, 1)
    part = torch.empty(lib.transoar_conv3d_wgrad_part_floats(k, nn_, chunks, 1), dtype=torch.float32, device=x.device)
    bias_part = torch.empty(chunks * nn_, dtype=torch.float32, device=x.device)
    dw = torch.empty((nn_, k), dtype=torch.float32, device=x.device)
    db = torch.empty(nn_, dtype=torch.float32, device=x.device)
    launch(lib.transoar_linear_wgrad_bias, x, gy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), bias_part.data_ptr(),
           db.data_ptr(), t, k, nn_, chunks)
    return dw, db
