"""CPU: conv_plan.plan_conv -- which kernels a 3x3x3 convolution layer runs, forward and both gradients, with every split-K
factor, chunk count and batch range -- is pure host arithmetic, so the dispatch policy is pinned here without a device.

The expected values were read off the dispatch as it stood at the commit before the plan existed, by a throw-away script
that called that commit's own predicates and arithmetic on the CPU (conv3d._use_gemm, conv_gemm._split_for(_tiles(...)),
_batch_chunks, wgrad_ring_supported, the budget lines of _wgrad, lds_wgrad_supported / c1_wgrad_supported on meta tensors
of the right layout, transoar_conv3d_k3_stat_rows) with the environment switches set through the module globals they were
read into.  None of them was read from conv_plan."""
import os

import pytest

from transoar_amd import _native, conv_plan
from transoar_amd.conv_plan import KNOBS, plan_conv

# (id, (n, cin, cout, d, h, w, stride), want_stats, switch turned off) ->
#     (fwd, dgrad, wgrad, split-K per batch range of fwd, of dgrad, weight-gradient partial tiles / workgroups / ring chunks
#      -- voxel_major: chunks per batch range --, stat_rows, launches per direction (fwd, dgrad, wgrad)); None: no plan
ROWS = [
    # tests/test_conv3d_gpu.py::test_conv3d_k3_flagship_layer_shapes; the last two (AMOS) need more than one batch range
    ('flagship0', (2, 1, 24, 160, 160, 256, 1), False, None, ('c1_halo', 'direct_flipped', 'c1_tr', (1,), (1,), 1024, 0, (1, 1, 1))),
    ('flagship1', (2, 24, 24, 160, 160, 256, 1), False, None, ('direct', 'direct_flipped', 'lds_tr', (1,), (1,), 512, 0, (1, 1, 1))),
    ('flagship2', (2, 24, 48, 160, 160, 256, 2), False, None, ('igemm', 's2_halo', 'ring', (1,), (1,), 85, 0, (1, 1, 1))),
    ('flagship3', (2, 48, 48, 80, 80, 128, 1), False, None, ('igemm', 'igemm_s1', 'ring', (1,), (1,), 85, 0, (1, 1, 1))),
    ('flagship4', (2, 48, 96, 80, 80, 128, 2), False, None, ('igemm', 's2_classes', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('flagship5', (2, 96, 96, 40, 40, 64, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('flagship6', (2, 96, 192, 40, 40, 64, 2), False, None, ('igemm', 's2_classes', 'voxel_major', (1,), (1,), (9,), 0, (1, 1, 1))),
    ('flagship7', (2, 192, 384, 20, 20, 32, 2), False, None, ('igemm', 's2_classes', 'voxel_major', (6,), (1,), (3,), 0, (2, 1, 1))),
    ('flagship8', (2, 384, 384, 10, 10, 16, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (6,), (6,), (3,), 0, (2, 2, 1))),
    ('flagship9', (2, 384, 768, 10, 10, 16, 2), False, None, ('igemm', 's2_classes', 'voxel_major', (16,), (6,), (1,), 0, (2, 2, 1))),
    ('flagship10', (2, 768, 768, 5, 5, 8, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (16,), (16,), (1,), 0, (2, 2, 1))),
    ('flagship11', (2, 96, 384, 40, 40, 64, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (1,), (1,), (12,), 0, (1, 1, 1))),
    ('flagship12', (2, 384, 384, 5, 5, 8, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (16,), (16,), (1,), 0, (2, 2, 1))),
    ('flagship13', (2, 24, 48, 256, 256, 128, 2), False, None, ('igemm', 's2_halo', 'ring', (1, 1), (1,), 85, 0, (2, 1, 1))),
    # 2^21 rows in two samples: the LDS weight gradient in four 32-channel blocks
    ('flagship14', (2, 48, 48, 128, 128, 64, 1), False, None, ('igemm', 'igemm_s1', 'lds_tr', (1, 1), (1, 1), 512, 0, (2, 2, 4))),
    # tests/test_conv3d_gpu.py::CASES
    ('conv3d0', (2, 24, 24, 6, 10, 16, 1), False, None, ('direct', 'direct_flipped', 'voxel_major', (1,), (1,), (1,), 0, (1, 1, 1))),
    ('conv3d1', (1, 24, 48, 8, 8, 16, 2), False, None, ('igemm', 's2_halo', 'voxel_major', (2,), (1,), (1,), 0, (2, 1, 1))),
    ('conv3d2', (2, 48, 96, 4, 6, 16, 2), False, None, ('igemm', 's2_classes', 'voxel_major', (5,), (3,), (1,), 0, (2, 2, 1))),
    ('conv3d3', (1, 96, 96, 5, 5, 8, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (10,), (10,), (1,), 0, (2, 2, 1))),
    ('conv3d4', (1, 96, 384, 4, 4, 8, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (10,), (16,), (1,), 0, (2, 2, 1))),
    ('conv3d5', (2, 8, 40, 3, 7, 24, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (1,), (4,), (1,), 0, (1, 2, 1))),
    ('conv3d6', (1, 1, 24, 6, 10, 16, 1), False, None, ('c1_padded', 'direct_flipped', 'c1', (1,), (1,), 15, 0, (1, 1, 1))),
    ('conv3d7', (1, 192, 64, 2, 2, 8, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (16,), (6,), (1,), 0, (2, 2, 1))),
    ('conv3d8', (2, 24, 24, 3, 4, 64, 1), False, None, ('direct', 'direct_flipped', 'lds_tr', (1,), (1,), 512, 0, (1, 1, 1))),
    ('conv3d9', (1, 8, 32, 2, 3, 128, 1), False, None, ('direct', 'direct_flipped', 'lds_tr', (1,), (1,), 512, 0, (1, 1, 1))),
    ('conv3d10', (1, 32, 16, 3, 2, 64, 1), False, None, ('igemm', 'igemm_s1', 'lds_tr', (3,), (1,), 512, 0, (2, 1, 1))),
    # more than 32 channels and 576 rows: the general voxel-major kernel, not the LDS one
    ('conv3d11', (1, 48, 48, 3, 3, 64, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (5,), (5,), (1,), 0, (2, 2, 1))),
    ('conv3d12', (1, 40, 64, 2, 2, 64, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (4,), (6,), (1,), 0, (2, 2, 1))),
    ('conv3d13', (2, 1, 32, 3, 4, 32, 1), False, None, ('c1_padded', 'direct_flipped', 'c1', (1,), (1,), 6, 0, (1, 1, 1))),
    ('conv3d14', (1, 1, 8, 2, 3, 48, 1), False, None, ('c1_padded', 'direct_flipped', 'c1', (1,), (1,), 2, 0, (1, 1, 1))),
    ('conv3d15', (3, 1, 24, 5, 3, 16, 1), False, None, ('c1_padded', 'direct_flipped', 'c1', (1,), (1,), 12, 0, (1, 1, 1))),
    ('conv3d16', (1, 24, 24, 18, 22, 200, 1), False, None, ('direct', 'direct_flipped', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('conv3d17', (1, 8, 32, 20, 30, 120, 1), False, None, ('direct', 'direct_flipped', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('conv3d18', (2, 16, 24, 17, 33, 136, 1), False, None, ('direct', 'direct_flipped', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('conv3d19', (1, 1, 24, 18, 30, 128, 1), False, None, ('c1_halo', 'direct_flipped', 'c1_tr', (1,), (1,), 540, 0, (1, 1, 1))),
    ('conv3d20', (2, 1, 24, 5, 7, 64, 1), False, None, ('c1_padded', 'direct_flipped', 'c1_tr', (1,), (1,), 70, 0, (1, 1, 1))),
    ('conv3d21', (1, 1, 32, 4, 6, 256, 1), False, None, ('c1_padded', 'direct_flipped', 'c1_tr', (1,), (1,), 24, 0, (1, 1, 1))),
    ('conv3d22', (2, 1, 8, 3, 5, 192, 1), False, None, ('c1_padded', 'direct_flipped', 'c1_tr', (1,), (1,), 30, 0, (1, 1, 1))),
    ('conv3d23', (1, 1, 16, 6, 4, 256, 1), False, None, ('c1_padded', 'direct_flipped', 'c1_tr', (1,), (1,), 24, 0, (1, 1, 1))),
    # tests/test_convgemm_gpu.py::CASES that the lists above do not hold; that test calls conv_gemm's functions directly,
    # Conv3dK3 leaves the shapes whose W / stride is no multiple of 8 to the stock convolution
    ('convgemm0', (2, 48, 48, 6, 10, 16, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (5,), (5,), (1,), 0, (2, 2, 1))),
    ('convgemm6', (1, 192, 136, 3, 5, 7, 1), False, None, None),
    ('convgemm7', (1, 200, 64, 5, 7, 9, 2), False, None, None),
    ('convgemm8', (1, 384, 768, 2, 4, 4, 2), False, None, None),
    ('convgemm9', (1, 768, 768, 2, 2, 4, 1), False, None, None),
    ('convgemm10', (2, 96, 192, 6, 6, 8, 2), False, None, None),
    ('convgemm11', (1, 56, 72, 7, 9, 11, 2), False, None, None),
    # the stage-0 layers as EncoderCnnBlock calls them, and layers the halo-tile kernel does not take
    ('stats_stem', (2, 1, 24, 160, 160, 256, 1), True, None, ('stats_halo', 'direct_flipped', 'c1_tr', (1,), (1,), 1024, 3200, (1, 1, 1))),
    ('stats_s0c2', (2, 24, 24, 160, 160, 256, 1), True, None, ('stats_halo', 'direct_flipped', 'lds_tr', (1,), (1,), 512, 3200, (1, 1, 1))),
    ('stats_not_covered', (2, 24, 24, 6, 10, 16, 1), True, None, ('direct', 'direct_flipped', 'voxel_major', (1,), (1,), (1,), 0, (1, 1, 1))),
    ('stats_gemm_layer', (1, 48, 32, 24, 32, 64, 1), True, None, ('igemm', 'igemm_s1', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('ring', (1, 48, 48, 16, 256, 64, 1), False, None, ('igemm', 'igemm_s1', 'ring', (1,), (1,), 85, 0, (1, 1, 1))),      # 2^18 rows
    ('igemm_no_split', (1, 48, 48, 24, 32, 64, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    # Cin = 1 with Cout > 32 or W % 16 != 0: the channels-first weight gradient
    ('channels_first_cout40', (1, 1, 40, 2, 3, 16, 1), False, None, ('c1_padded', 'direct_flipped', 'channels_first', (1,), (1,), 0, 0, (1, 1, 1))),
    ('channels_first_w24', (1, 1, 8, 2, 3, 24, 1), False, None, ('c1_padded', 'direct_flipped', 'channels_first', (1,), (1,), 0, 0, (1, 1, 1))),
    # a short last batch range has a split and a chunk count of its own
    ('uneven_last_range', (1025, 48, 48, 4, 8, 64, 1), False, None, ('igemm', 'igemm_s1', 'lds_tr', (1, 5), (1, 5), 512, 0, (3, 3, 4))),
    ('uneven_voxel_major', (1025, 48, 48, 4, 16, 32, 1), False, None, ('igemm', 'igemm_s1', 'voxel_major', (1, 5), (1, 5), (37, 4), 0, (3, 3, 2))),
    # one row per environment switch, switched off
    ('off_c1_wgrad_tr', (2, 1, 24, 5, 7, 64, 1), False, 'c1_wgrad_tr', ('c1_padded', 'direct_flipped', 'c1', (1,), (1,), 18, 0, (1, 1, 1))),
    ('off_wgrad_tr', (2, 24, 24, 3, 4, 64, 1), False, 'wgrad_tr', ('direct', 'direct_flipped', 'lds', (1,), (1,), 512, 0, (1, 1, 1))),
    ('off_dgrad_s2_halo', (1, 24, 48, 8, 8, 16, 2), False, 'dgrad_s2_halo', ('igemm', 's2_classes', 'voxel_major', (2,), (1,), (1,), 0, (2, 1, 1))),
    ('off_wgrad_ring', (1, 48, 48, 16, 256, 64, 1), False, 'wgrad_ring', ('igemm', 'igemm_s1', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
    ('off_conv_stats', (1, 24, 24, 18, 22, 200, 1), True, 'conv_stats', ('direct', 'direct_flipped', 'voxel_major', (1,), (1,), (18,), 0, (1, 1, 1))),
]
ALL_ON = conv_plan.Knobs(True, True, True, True, True)


def _plan(shape, want_stats, off):
    return plan_conv(*shape, want_stats, ALL_ON._replace(**{off: False}) if off else ALL_ON)


@pytest.mark.parametrize("name,shape,want_stats,off,want", ROWS, ids=[r[0] for r in ROWS])
def test_plan_chooses_what_the_dispatch_chose(name, shape, want_stats, off, want):
    plan = _plan(shape, want_stats, off)
    if want is None:
        assert plan is None
        return
    wgrad = tuple(c for _, _, c in plan.wgrad_ranges) if plan.wgrad == "voxel_major" else plan.wgrad_parts
    got = (plan.fwd, plan.dgrad, plan.wgrad, tuple(s for _, _, s in plan.fwd_ranges), tuple(s for _, _, s in plan.dgrad_ranges),
           wgrad, plan.stat_rows, tuple(len(plan.launches(k)) for k in ("fwd", "dgrad", "wgrad")))
    assert got == want
    assert plan.stride == shape[6] and plan.packs == (plan.fwd == "igemm")
    for ranges in (plan.fwd_ranges, plan.dgrad_ranges, plan.wgrad_ranges):          # the ranges tile the batch in order
        assert not ranges or [i for i, _, _ in ranges] == [sum(c for _, c, _ in ranges[:k]) for k in range(len(ranges))]
        assert not ranges or sum(c for _, c, _ in ranges) == shape[0]


def test_lds_weight_gradient_block_list():
    assert _plan((2, 48, 48, 128, 128, 64, 1), False, None).wgrad_blocks == ((0, 32, 0, 32), (0, 32, 32, 16), (32, 16, 0, 32), (32, 16, 32, 16))
    assert _plan((1, 8, 32, 2, 3, 128, 1), False, None).wgrad_blocks == ((0, 32, 0, 8),)
    assert _plan((2, 48, 48, 80, 80, 128, 1), False, None).wgrad_blocks == ()


def test_launch_order_of_split_and_batch_ranges():
    plan = _plan((1025, 48, 48, 4, 16, 32, 1), False, None)
    assert plan.launches("fwd") == ["transoar_conv3d_igemm", "transoar_conv3d_igemm", "transoar_conv3d_finish"]
    assert plan.launches("dgrad") == plan.launches("fwd")
    assert plan.launches("wgrad") == ["transoar_conv3d_wgrad"] * 2


@pytest.mark.parametrize("shape", [(2, 12, 24, 4, 4, 16, 1), (2, 24, 20, 4, 4, 16, 1), (1, 1, 24, 8, 8, 16, 2), (1, 1, 72, 4, 4, 16, 1),
                                   (1, 24, 48, 8, 8, 24, 2), (1, 24, 24, 4, 4, 12, 1), (1, 24, 48, 7, 8, 16, 2), (1, 24, 48, 8, 9, 16, 2),
                                   (1, 24, 48, 8, 8, 16, 3)])
def test_no_plan_outside_the_kernels_domain(shape):
    """Odd channel counts, Cin = 1 with stride 2 or more than 64 outputs, W / stride no multiple of 8, odd extents with
    stride 2: the layer stays on the stock convolution."""
    assert plan_conv(*shape) is None


def test_one_sample_past_the_row_limit_raises():
    """2^21 rows in ONE sample: the implicit-GEMM forward cannot split the batch, and said so before the plan existed."""
    with pytest.raises(RuntimeError, match="one sample has 2097152 rows"):
        plan_conv(1, 48, 48, 128, 256, 64, 1)


def test_launches_name_declared_entry_points():
    declared = set()
    for header in ("transoar_conv3d.h", "transoar_convgemm.h"):
        with open(os.path.join(_native._INCLUDE, header)) as f:
            declared |= set(_native.parse_header(f.read(), header))
    for name, shape, want_stats, off, want in ROWS:
        plan = _plan(shape, want_stats, off)
        for direction in ("fwd", "dgrad", "wgrad") if plan else ():
            names = plan.launches(direction)
            assert names and set(names) <= declared, (name, direction, names)


def test_plan_is_cached():
    assert plan_conv(2, 96, 96, 40, 40, 64, 1) is plan_conv(2, 96, 96, 40, 40, 64, 1)
    assert plan_conv(2, 96, 96, 40, 40, 64, 1, False, KNOBS) is plan_conv(2, 96, 96, 40, 40, 64, 1, False, KNOBS)

