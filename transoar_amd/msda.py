"""The ``MSDA`` object: the two functions the reference's pybind module
``MultiScaleDeformableAttention`` exports (ops/src/vision.cpp:13-16), bound to
the gfx950 C ABI instead of the CUDA extension.

    import transoar_amd.msda as MSDA
    out = MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, attn, im2col_step)
    gv, gl, ga = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, attn, grad_out, im2col_step)

Argument order, layouts, the contiguity / device checks and the returned shapes
follow ops/src/cuda/ms_deform_attn_cuda.cu:20-80 (forward) and :83-154
(backward).  Differences: bf16/f16 storage is accepted (fp32 accumulate; the
reference dispatches float/double only, .cu:64), kernel launch errors raise
(the reference printf()s them, ms_deform_im2col_cuda.cuh:1119-1123), and
``im2col_step`` only takes part in the reference's divisibility check -- the
batch is processed in one launch.
"""
import ctypes
import os

import torch

from . import _native

_DT = {torch.float32: _native.F32, torch.float64: _native.F64,
       torch.bfloat16: _native.BF16, torch.float16: _native.F16}

# bit set forwarded to the C ABI (see include/transoar_msda3d.h); module-level so
# tests can force the generic kernels.
flags = int(os.environ.get("TRANSOAR_MSDA_FLAGS", "0"))
DETERMINISTIC = 64      # TRANSOAR_MSDA3D_DETERMINISTIC
ERR_MODE = -8           # TRANSOAR_ERR_MODE
# Bit-stable backward ("deterministic-mode backward"): grad_value is accumulated in an order that does not depend
# on atomics (stable sort of the points by (cell, point index), brick-owner walk on every level) -- about 4x the default
# backward's time.  On when this switch is set (strict: a form the mode does not cover raises) or when
# torch.use_deterministic_algorithms(True) is in force (a form that is not covered raises like torch's own ops do, or warns
# and runs the default order under warn_only=True).  grad_sampling_loc / grad_attn_weight and the forward have no atomics.
deterministic = os.environ.get("TRANSOAR_MSDA_DETERMINISTIC", "0") == "1"


# host copy of a spatial_shapes tensor, kept ON the tensor object (it dies with it; an address-keyed
# cache would hand a recycled allocation the shapes of a dead tensor): the reference passes the level
# shapes as a device tensor only; one .tolist() (a sync) per distinct tensor buys the brick schedule
# of the kernels.  locality_hint = False skips it; the per-brick kernels then fall back to the
# per-item ones (same results).
locality_hint = True


def _shapes_on_host(spatial_shapes):
    if not locality_hint:
        return None, None
    hit = getattr(spatial_shapes, "_transoar_host_shapes", None)
    if hit is None or hit[0] != spatial_shapes._version:
        vals = [int(v) for v in spatial_shapes.flatten().tolist()]
        hit = (spatial_shapes._version, (ctypes.c_int64 * len(vals))(*vals))
        spatial_shapes._transoar_host_shapes = hit
    return hit[1], ctypes.addressof(hit[1])


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _check_inputs(named):
    for name, t in named:
        _require(t.is_contiguous(), "%s tensor has to be contiguous" % name)
    if not named[0][1].is_cuda:
        # ops/src/ms_deform_attn.h:38,60
        raise RuntimeError("Not implemented on the CPU")
    dev = named[0][1].device
    for name, t in named:
        _require(t.is_cuda and t.device == dev, "%s must be a CUDA tensor on %s" % (name, dev))


def _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
    _require(value.dim() == 4, "value must be (N, S, M, C)")
    _require(sampling_loc.dim() == 6 and sampling_loc.size(-1) == 3,
             "sampling_loc must be (N, Lq, M, L, P, 3)")
    N, S, M, C = value.shape
    L = spatial_shapes.size(0)
    Lq, P = sampling_loc.size(1), sampling_loc.size(4)
    _require(spatial_shapes.dtype == torch.int64 and tuple(spatial_shapes.shape) == (L, 3),
             "spatial_shapes must be int64 (L, 3)")
    _require(level_start_index.dtype == torch.int64 and tuple(level_start_index.shape) == (L,),
             "level_start_index must be int64 (L,)")
    _require(tuple(sampling_loc.shape) == (N, Lq, M, L, P, 3), "sampling_loc shape mismatch")
    _require(tuple(attn_weight.shape) == (N, Lq, M, L, P), "attn_weight shape mismatch")
    step = min(N, int(im2col_step))
    _require(step > 0 and N % step == 0,
             "batch(%d) must divide im2col_step(%d)" % (N, step))      # .cu:52
    _require(value.dtype in _DT, "unsupported value dtype %s" % value.dtype)
    return N, S, M, C, L, Lq, P


def _coerce_loc(value, sampling_loc, attn_weight):
    # bf16/f16 value may come with fp32 locations (what autocast produces) or
    # with same-dtype locations; anything else is converted to fp32 / value dtype.
    half = value.dtype in (torch.bfloat16, torch.float16)
    if sampling_loc.dtype != attn_weight.dtype or not (
            sampling_loc.dtype == value.dtype or (half and sampling_loc.dtype == torch.float32)):
        want = torch.float32 if half else value.dtype
        sampling_loc = sampling_loc.to(want).contiguous()
        attn_weight = attn_weight.to(want).contiguous()
    return sampling_loc, attn_weight


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                           im2col_step):
    """-> Tensor (N, Lq, M*C); replaces ops/src/ms_deform_attn.h:20-39."""
    _check_inputs([("value", value), ("spatial_shapes", spatial_shapes),
                   ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
                   ("attn_weight", attn_weight)])
    N, S, M, C, L, Lq, P = _dims(value, spatial_shapes, level_start_index, sampling_loc,
                                 attn_weight, im2col_step)
    sampling_loc, attn_weight = _coerce_loc(value, sampling_loc, attn_weight)
    out = torch.empty((N, Lq, M * C), dtype=value.dtype, device=value.device)
    _keep, host_ptr = _shapes_on_host(spatial_shapes)
    _native.launch(_native.lib.transoar_msda3d_forward, value,
                   value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                   sampling_loc.data_ptr(), attn_weight.data_ptr(), out.data_ptr(),
                   N, S, M, C, L, Lq, P, _DT[value.dtype], _DT[sampling_loc.dtype], host_ptr, flags)
    return out


def ms_deform_attn_forward_fused(value, spatial_shapes, proj, reference_points):
    """Gather with the module's sampling head in its prologue (no reference counterpart as one call: it is
    ops/modules/ms_deform_attn.py:114-136 -- softmax, ``ref + offsets / (W, H, D)``, MSDeformAttnFunction -- without
    materialising sampling_locations / attention_weights).

    value (N, S, M, C) bf16/f16; proj (N, S, 4*M*L*P) bf16 = [offsets (M, L, P, 3) | logits (M, L*P)] per query;
    reference_points (1 or N, S, L, 3) fp32.  -> (N, S, M*C).  Queries are the pyramid's voxels (Lq == S)."""
    _check_inputs([("value", value), ("spatial_shapes", spatial_shapes), ("proj", proj),
                   ("reference_points", reference_points)])
    _require(value.dim() == 4 and value.dtype in (torch.bfloat16, torch.float16), "value must be 16-bit (N, S, M, C)")
    N, S, M, C = value.shape
    L = spatial_shapes.size(0)
    P = proj.size(-1) // (4 * M * L)
    _require(proj.dtype == torch.bfloat16 and tuple(proj.shape) == (N, S, 4 * M * L * P), "proj must be bf16 (N, S, 4*M*L*P)")
    _require(reference_points.dtype == torch.float32 and reference_points.dim() == 4 and
             tuple(reference_points.shape[1:]) == (S, L, 3) and reference_points.size(0) in (1, N),
             "reference_points must be fp32 (1 or N, S, L, 3)")
    out = torch.empty((N, S, M * C), dtype=value.dtype, device=value.device)
    _keep, host_ptr = _shapes_on_host(spatial_shapes)
    _require(host_ptr is not None, "the fused gather needs the level shapes on the host (locality_hint)")
    _native.launch(_native.lib.transoar_msda3d_forward_fused, value,
                   value.data_ptr(), proj.data_ptr(), reference_points.data_ptr(), reference_points.size(0) * S,
                   out.data_ptr(), N, S, M, C, L, P, _DT[value.dtype], host_ptr)
    return out          # a form the kernel does not cover raises (TRANSOAR_ERR_DIM): ask plan() first


PLAN_FIELDS = ("fwd", "bwd_query", "bwd_value", "coarse_first")          # TRANSOAR_PLAN_* of the header
FWD_PCM, FWD_Q16 = 4, 5                                                  # TRANSOAR_FWD_PCM / _Q16: the point-column gathers


def plan(value, spatial_shapes, Lq, P, loc_dtype, grad_proj=False, call_flags=None):
    """-> (status, {field: kernel code}) of transoar_msda3d_plan: the kernels the forward and the backward (grad_proj: the
    backward_proj entry) launch for this form and these flags (default: the module's).  Host arithmetic only.  status: 0,
    ERR_MODE (the backward refuses the form) or an argument error, after which every field is 0."""
    N, S, M, C = value.shape
    _keep, host_ptr = _shapes_on_host(spatial_shapes)
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    rc = _native.lib.transoar_msda3d_plan(N, S, M, C, spatial_shapes.size(0), Lq, P, _DT[value.dtype], _DT[loc_dtype],
                                          host_ptr, flags if call_flags is None else call_flags, int(grad_proj), out)
    return rc, dict(zip(PLAN_FIELDS, out))


def _backward_dims(tensors, im2col_step):
    """The input checks of both backward entries; tensors = (value, shapes, starts, loc, attn, grad_output)."""
    _check_inputs(list(zip(("value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "grad_output"), tensors)))
    N, S, M, C, L, Lq, P = dims = _dims(*tensors[:5], im2col_step)
    _require(tuple(tensors[5].shape) == (N, Lq, M * C) and tensors[5].dtype == tensors[0].dtype,
             "grad_output must be (N, Lq, M*C) with value's dtype")
    return dims


def _backward(fn, tensors, grads, dims, call_flags):
    """The launch of both backward entries: the workspace for `call_flags`, then ONE call of fn(*tensors, *grads, ...)."""
    value, spatial_shapes, sampling_loc = tensors[0], tensors[1], tensors[3]
    dims = (*dims, _DT[value.dtype], _DT[sampling_loc.dtype])
    _keep, host_ptr = _shapes_on_host(spatial_shapes)
    ws_bytes = _native.lib.transoar_msda3d_backward_workspace_bytes(*dims, call_flags)
    workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=value.device)
    _native.launch(fn, value, *[t.data_ptr() for t in tensors], *[g.data_ptr() for g in grads],
                   workspace.data_ptr(), ws_bytes, *dims, host_ptr, call_flags)
    return grads


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                            grad_output, im2col_step):
    """-> [grad_value, grad_sampling_loc, grad_attn_weight]; replaces
    ops/src/ms_deform_attn.h:41-61."""
    dims = _backward_dims((value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output), im2col_step)
    loc_in_dtype, attn_in_dtype = sampling_loc.dtype, attn_weight.dtype
    sampling_loc, attn_weight = _coerce_loc(value, sampling_loc, attn_weight)
    call_flags = flags
    strict = deterministic or bool(flags & DETERMINISTIC)          # the switch itself: an uncovered form raises
    if strict or torch.are_deterministic_algorithms_enabled():
        call_flags = flags | DETERMINISTIC
        if plan(value, spatial_shapes, dims[5], dims[6], sampling_loc.dtype, call_flags=call_flags)[0] == ERR_MODE:
            if strict:
                _native.check(ERR_MODE, "transoar_msda3d_backward")
            if not torch.is_deterministic_algorithms_warn_only_enabled():
                raise RuntimeError("ms_deform_attn_backward does not have a deterministic implementation for this form (16-bit "
                                   "storage, 64 channels, 4 points, <= 4 levels with queries = the pyramid's voxels are covered), "
                                   "but torch.use_deterministic_algorithms(True) is set; use warn_only=True to run the default order")
            import warnings
            warnings.warn("ms_deform_attn_backward: no deterministic implementation for this form; running the default "
                          "(atomic-order dependent) accumulation")
            call_flags = flags
    gv, gl, ga = _backward(_native.lib.transoar_msda3d_backward,
                           (value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output),
                           [torch.empty_like(value), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)], dims, call_flags)
    return [gv, gl.to(loc_in_dtype), ga.to(attn_in_dtype)]


def ms_deform_attn_backward_proj(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step):
    """-> [grad_value, grad_proj] or None: the backward with the sampling head's backward folded into the query kernel
    (transoar_msda3d_backward_proj): grad_proj (N, Lq, 4*M*L*P) bf16 is the gradient of the stacked [sampling_offsets |
    attention_weights] projection.  None, without a launch, when the plan says the form is not covered: the caller then
    runs ms_deform_attn_backward and the head's own backward kernel."""
    tensors = (value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output)
    N, S, M, C, L, Lq, P = dims = _backward_dims(tensors, im2col_step)
    call_flags = flags | (DETERMINISTIC if (deterministic or torch.are_deterministic_algorithms_enabled()) else 0)
    if attn_weight.dtype != sampling_loc.dtype or plan(value, spatial_shapes, Lq, P, sampling_loc.dtype, True, call_flags)[0] != 0:
        return None
    grads = [torch.empty_like(value), torch.empty((N, Lq, 4 * M * L * P), dtype=torch.bfloat16, device=value.device)]
    return _backward(_native.lib.transoar_msda3d_backward_proj, tensors, grads, dims, call_flags)
