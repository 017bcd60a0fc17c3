"""ctypes binding and autograd shim of the dense head-dimension-48 cross-attention kernels (C ABI:
include/transoar_denseattn.h; kernels: csrc/dense_attn.hip).

Reference semantics: the dense branch of FocusedAttn.forward, necks/focused_decoder.py:228-262 -- per (batch, head)

    O = softmax(mask(scale Q_h K_h^T)) V_h,      Q (B, Nq, 384), K / V (B, L, 384), heads = 48-column slices in place,

with the layer's boolean (Nq, L) mask given as per-organ key words (the queries of an organ share one row).
Forward is one kernel (plus a small combine pass when the keys are split across workgroups); the backward recomputes P
from the saved log-sum-exp: one kernel for dQ, one for dK / dV (no atomics).  No fallback: the library must be built.
"""
import os

import torch

from . import _native
from ._native import launch

ABI_VERSION = 1
CHANNELS = 384
HEADS = 8
lib = _native.bind("denseattn", abi=ABI_VERSION)
ENABLED = os.environ.get("TRANSOAR_DENSE_FUSED", "1") != "0"


def _key_bits(attn_mask, n_org):
    n_q, n_keys = attn_mask.shape
    if not bool(attn_mask.any()):
        return None
    if n_org < 1 or n_q % n_org:
        raise ValueError("dense_attn.key_bits: %d queries are not a multiple of %d organs" % (n_q, n_org))
    rows = attn_mask.view(n_org, n_q // n_org, n_keys)
    if not bool((rows == rows[:, :1]).all()):
        raise ValueError("dense_attn.key_bits: the queries of an organ do not share one mask row")
    pad = rows[:, 0]
    if bool(pad.all(1).any()):
        raise ValueError("dense_attn.key_bits: an organ has no key to attend to (the reference yields NaN there)")
    tiles = (n_keys + 31) // 32
    full = torch.ones(n_org, tiles * 32, dtype=torch.bool, device=pad.device)
    full[:, :n_keys] = pad
    weights = (1 << torch.arange(32, dtype=torch.int64, device=pad.device))
    words = (full.view(n_org, tiles, 32).to(torch.int64) * weights).sum(-1)
    words = torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32).contiguous()
    live_tile = ~full.view(n_org, tiles, 32).all(-1)                       # the tile holds a live key
    index = torch.arange(tiles, device=pad.device)
    first = torch.where(live_tile, index, tiles).amin(1)
    last = torch.where(live_tile, index + 1, 0).amax(1)
    bounds = torch.stack((first, last), 1).to(torch.int32).contiguous()
    return words, bounds, n_q // n_org


def key_bits(attn_mask, n_org):
    """attn_mask (Nq, L) bool, True = masked, organ-major rows -> None when nothing is masked, else (keybits
    (O, ceil(L/32)) int32: bit i of word t = key 32 t + i is masked, the bits past L set; bounds (O, 2) int32: [first, last)
    32-key tile that holds a live key; rows per organ).  Raises ValueError when the queries of an organ do not share
    one row or an organ has no key.  Cached on the tensor per (address, version), like roi_attn.key_mask: entries are
    only ever ADDED (a captured graph may hold the address of an older entry's tensors)."""
    key = (attn_mask.data_ptr(), attn_mask._version, str(attn_mask.device), tuple(attn_mask.shape), n_org)
    cache = getattr(attn_mask, "_transoar_key_bits", None)
    hit = None if cache is None else cache.get(key)
    if hit is None:
        try:
            hit = ("ok", _key_bits(attn_mask, n_org))
        except ValueError as refusal:
            hit = ("refused", str(refusal))
        try:
            if cache is None:
                cache = attn_mask._transoar_key_bits = {}
            cache[key] = hit
        except Exception:        # noqa: BLE001  (a tensor subclass that refuses attributes: just do not cache)
            pass
    if hit[0] == "refused":
        raise ValueError(hit[1])
    return hit[1]


def usable(q, k, v, n_heads):
    """Can the kernels take this attention?  bf16 on the GPU, dense (B, Nq / L, 384) operands, 8 heads, 32-bit
    addressable buffers."""
    return (ENABLED and q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
            and n_heads == HEADS and q.dim() == 3 and k.dim() == 3 and q.shape[-1] == CHANNELS and k.shape[-1] == CHANNELS
            and k.shape == v.shape and q.shape[0] == k.shape[0] and q.shape[1] > 0 and k.shape[1] > 0
            and q.shape[0] * HEADS <= 65535 and max(q.numel(), k.numel()) * 2 < (1 << 31) - 1
            and q.shape[0] * HEADS * q.shape[1] * 4 * (1 + 16 * 50) < (1 << 31) - 1)


def pick_split(batch, n_q, n_keys):
    """Key splits so that the forward / dQ grid (splits x query blocks of 64 x batch x heads) is about four workgroups
    per CU (256 CUs; a workgroup holds a quarter of a CU's registers), never more than there are 64-key stages."""
    blocks = batch * HEADS * ((n_q + 63) // 64)
    return max(1, min(16, 1024 // max(blocks, 1), (n_keys + 63) // 64))


class DenseAttention(torch.autograd.Function):
    """(out, lse) = attention of q (B, Nq, 384) over k / v (B, L, 384) per 48-channel head; bits = key_bits(...) or None."""

    @staticmethod
    def forward(ctx, q, k, v, bits, scale, n_split):
        b, n_q, c = q.shape
        n_keys = k.shape[1]
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        words, bounds, rpo = bits if bits is not None else (None, None, n_q)
        if words is not None and (words.device != q.device or words.shape[1] != (n_keys + 31) // 32):
            raise ValueError("dense_attn: the key words do not belong to these keys")
        split = n_split or pick_split(b, n_q, n_keys)
        out = torch.empty_like(q)
        lse = torch.empty((b, HEADS, n_q), dtype=torch.float32, device=q.device)
        ws_bytes = lib.transoar_dense_attn_workspace_bytes(b, n_q, split)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        n_org = n_q // rpo
        launch(lib.transoar_dense_attn_forward, q, q.data_ptr(), k.data_ptr(), v.data_ptr(), _native.ptr(words),
               _native.ptr(bounds), out.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws_bytes, b, n_q, n_keys, c, HEADS,
               n_org, rpo, scale, split)
        ctx.save_for_backward(q, k, v, out, lse, words, bounds)
        ctx.args = (n_org, rpo, scale, split)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, d_out, _d_lse):
        q, k, v, out, lse, words, bounds = ctx.saved_tensors
        n_org, rpo, scale, split = ctx.args
        b, n_q, c = q.shape
        n_keys = k.shape[1]
        d_out = d_out.to(torch.bfloat16).contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws_bytes = lib.transoar_dense_attn_workspace_bytes(b, n_q, split)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        launch(lib.transoar_dense_attn_backward, q, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), d_out.data_ptr(),
               lse.data_ptr(), _native.ptr(words), _native.ptr(bounds), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
               ws.data_ptr(), ws_bytes, b, n_q, n_keys, c, HEADS, n_org, rpo, scale, split)
        return dq, dk, dv, None, None, None


def dense_attention(q, k, v, bits=None, scale=None, n_split=None, return_lse=False):
    scale = float(scale) if scale is not None else (q.shape[-1] // HEADS) ** -0.5
    out, lse = DenseAttention.apply(q, k, v, bits, scale, n_split)
    return (out, lse) if return_lse else out
