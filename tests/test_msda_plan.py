"""CPU: transoar_msda3d_plan -- which kernels the MSDeformAttn-3D entry points launch for a shape, dtypes and flags -- is
pure host arithmetic (transoar_amd/csrc/msda3d_plan.hpp), so the dispatch policy is pinned here without a device.  The
expected kernels were read off the dispatch code as it stood before the plan existed; the only deliberate difference is
that TRANSOAR_MSDA3D_DETERMINISTIC on a form of the generic kernels is refused (it used to run the atomic scatter).
The workspace sizes are literals recorded from the library built at the commit before the plan was introduced: the
refactor must not change them."""
import ctypes

import pytest

from transoar_amd import _native

F32, F64, BF16 = _native.F32, _native.F64, _native.BF16
ERR_MODE = -8
FWD = {"generic": 0, "vec": 1, "brick": 2, "mma": 3, "pcm": 4, "q16": 5}
QUERY = {"generic": 0, "vec": 1, "brick": 2, "mma": 3, "mma_det": 4}
VALUE = {"generic": 0, "pull": 1, "tile_w8": 2, "tile_mma": 3}
A = [(9, 6, 11), (5, 3, 6), (2, 2, 3)]
B = [(8, 8, 16), (4, 4, 8), (2, 2, 4), (1, 1, 2)]


def plan(levels=A, N=2, M=6, C=64, P=4, Lq=None, vdt=BF16, ldt=F32, host=True, flags=0, grad_proj=0):
    """-> (rc, [fwd, query, value, coarse_first], workspace bytes) of the library for one row of the table."""
    S = sum(d * h * w for d, h, w in levels)
    flat = [int(x) for lvl in levels for x in lvl]
    shapes = (ctypes.c_int64 * len(flat))(*flat)
    dims = (N, S, M, C, len(levels), Lq or S, P, vdt, ldt)
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = _native.lib.transoar_msda3d_plan(*dims, ctypes.addressof(shapes) if host else None, flags, grad_proj, out)
    return rc, list(out), _native.lib.transoar_msda3d_backward_workspace_bytes(*dims, flags)


# (id, arguments, fwd, query, value, coarse_first, workspace bytes at the parent commit)
ROWS = [
    ("defaults", {}, "pcm", "mma", "tile_mma", 2, 6414496),
    ("q16", dict(flags=128), "q16", "mma", "tile_mma", 2, 6414496),
    ("mma_q32", dict(flags=32), "mma", "mma", "tile_mma", 2, 6414496),
    ("no_mma", dict(flags=16), "brick", "brick", "tile_w8", 2, 6414496),
    ("no_brick", dict(flags=4), "vec", "vec", "pull", 3, 6414496),
    ("force_generic", dict(flags=1), "generic", "generic", "generic", 3, 2138112),
    ("deterministic", dict(flags=64), "pcm", "mma_det", "tile_mma", 3, 41672736),      # no coarse level in this mode
    ("loc_bf16", dict(ldt=BF16), "mma", "mma", "tile_mma", 2, 6414496),
    ("no_host_shapes", dict(host=False), "vec", "vec", "pull", 3, 6414496),
    ("Lq50", dict(Lq=50), "vec", "vec", "tile_mma", 3, 2693536),                        # 200 points < 32 * 12 voxels
    ("P2", dict(P=2), "vec", "vec", "tile_mma", 2, 4410016),
    ("C128", dict(C=128), "vec", "vec", "pull", 3, 8552608),
    ("C32", dict(C=32), "generic", "generic", "generic", 3, 1069056),
    ("fp32", dict(vdt=F32, ldt=F32), "vec", "vec", "tile_w8", 2, 6414496),
    ("fp64_C64", dict(vdt=F64, ldt=F64), "vec", "vec", "pull", 3, 9621664),
    ("fp64_C5", dict(vdt=F64, ldt=F64, C=5), "generic", "generic", "generic", 3, 0),
    ("five_levels", dict(levels=A + [(1, 1, 2), (1, 1, 1)]), "brick", "brick", "tile_mma", 2, 9126304),
    # 4 * 1001 points < 32 * 1001 voxels: the only level stays on the tile walk
    ("one_long_level", dict(levels=[(1, 1, 1001)]), "brick", "brick", "tile_mma", 1, 5381584),
    # 4 * 1170 = 4680 points per head: >= 32 * 128 voxels of level 1, < 32 * 1024 of level 0
    ("B_grad_proj", dict(levels=B, grad_proj=1), "pcm", "mma", "tile_mma", 1, 13029360),
]
# (id, arguments, fwd): forms the backward refuses with TRANSOAR_ERR_MODE; the forward field is filled all the same
REFUSED = [
    ("fp32_deterministic", dict(vdt=F32, ldt=F32, flags=64), "vec"),
    ("fp64_C5_deterministic", dict(vdt=F64, ldt=F64, C=5, flags=64), "generic"),        # the deliberate change
    ("A_grad_proj", dict(grad_proj=1), "pcm"),                                          # L * P != 16
    ("B_grad_proj_no_mma", dict(levels=B, grad_proj=1, flags=16), "brick"),
    ("B_grad_proj_loc_bf16", dict(levels=B, grad_proj=1, ldt=BF16), "mma"),
]


@pytest.mark.parametrize("name,args,fwd,query,value,coarse_first,ws_bytes", ROWS, ids=[r[0] for r in ROWS])
def test_plan_chooses_what_the_dispatch_chose(name, args, fwd, query, value, coarse_first, ws_bytes):
    rc, fields, ws = plan(**args)
    assert rc == 0
    assert fields == [FWD[fwd], QUERY[query], VALUE[value], coarse_first]
    assert ws == ws_bytes


@pytest.mark.parametrize("name,args,fwd", REFUSED, ids=[r[0] for r in REFUSED])
def test_plan_refuses_uncovered_forms(name, args, fwd):
    rc, fields, _ = plan(**args)
    assert rc == ERR_MODE
    assert fields == [FWD[fwd], -1, -1, -1]


def test_plan_argument_errors():
    out = (ctypes.c_int * 4)()
    f = _native.lib.transoar_msda3d_plan
    assert f(2, 696, 6, 64, 3, 696, 4, BF16, F32, None, 0, 0, None) == -1
    assert f(2, 696, 6, 0, 3, 696, 4, BF16, F32, None, 0, 0, out) == -2
    assert f(2, 696, 6, 64, 3, 696, 4, F32, F64, None, 0, 0, out) == -3
    assert f(2, 696, 6, 64, 9, 696, 4, BF16, F32, None, 0, 0, out) == -5
