"""Which kernels a 3x3x3 convolution layer runs: forward, data gradient and weight gradient, chosen from the layer's shape
alone.  Pure host arithmetic: no tensor, no HIP call (transoar_conv3d_k3_stat_rows is host arithmetic inside the library).
conv3d.py and conv_gemm.py are the launchers: they switch on what ``plan_conv`` says and take every split, chunk count and
batch range from here.  A new route is one more value of ``fwd`` / ``dgrad`` / ``wgrad`` and one row of
tests/test_conv_plan.py."""
import functools
import os
from typing import NamedTuple


class Knobs(NamedTuple):
    """The A/B switches of the convolution routes (environment, read once; all on by default)."""
    c1_wgrad_tr: bool       # TRANSOAR_C1_WGRAD_TR: Cin = 1 weight gradient with coalesced loads + transposing LDS reads
    wgrad_tr: bool          # TRANSOAR_WGRAD_TR: second LDS weight gradient, transposing LDS reads, 4 waves (conv3d_wgrad_tr.hpp)
    dgrad_s2_halo: bool     # TRANSOAR_DGRAD_S2_HALO: the halo-tile stride-2 data gradient (conv_dgrad_s2.hpp)
    wgrad_ring: bool        # TRANSOAR_WGRAD_RING: the LDS-ring weight gradient (conv_wgrad_ring.hpp)
    conv_stats: bool        # TRANSOAR_CONV_STATS: InstanceNorm statistics in the epilogue of the halo-tile forward


def _on(name):
    return os.environ.get(name, "1") != "0"


KNOBS = Knobs(_on("TRANSOAR_C1_WGRAD_TR"), _on("TRANSOAR_WGRAD_TR"), _on("TRANSOAR_DGRAD_S2_HALO"), _on("TRANSOAR_WGRAD_RING"),
              _on("TRANSOAR_CONV_STATS"))

# launches with fewer output tiles than this split their K steps (per-split partial maps + a finish pass)
SPLIT_BELOW_TILES = 384
MAX_ROWS = 1 << 21          # rows (voxels of the row space) per launch: the kernels decompose a row index with float reciprocals
WGRAD_BLOCKS = 512          # workgroups of a weight-gradient launch: one resident set (2 per CU); 2x for very long or very wide problems
WGRAD_RING_CHUNKS = 85      # workgroups per filter plane of a ring launch: 3 x 85 = one 512-thread workgroup per CU
C1_WGRAD_PARTIALS = 3200
C1_WGRAD_TR_PARTIALS = 1024         # persistent: 4 workgroups per CU
LDS_WGRAD_GROUPS = 512
LDS_WGRAD_TR_GROUPS = 512           # 2 workgroups per CU (202 VGPRs), 2 waves per SIMD


def use_gemm(cin, cout, stride):
    """Which forward / data-gradient kernel family: the LDS-tiled implicit GEMM from 48 channels up and for every strided
    layer with >= 8 input channels; the halo-tile / direct kernels of conv3d.hip for the full-resolution 24-channel layers."""
    return cin >= 8 and cin % 8 == 0 and cout % 8 == 0 and (stride == 2 or cin > 24 or cout > 32)


def batch_ranges(n, rows_per_sample, what):
    """Batch ranges [(first, count), ...] whose row count stays below MAX_ROWS (one range when the whole batch fits).
    A channels-last (N, C, D, H, W) tensor sliced along N is still a dense channels-last tensor, so a range is just
    another launch on a view.  AMOS at its reference batch (2 x 128 x 128 x 64 = 2^21 rows at stage 1) needs this."""
    if n * rows_per_sample < MAX_ROWS:
        return [(0, n)]
    per = (MAX_ROWS - 1) // rows_per_sample
    if per < 1:
        raise RuntimeError("%s: one sample has %d rows, the implicit-GEMM kernels address < %d per launch"
                           % (what, rows_per_sample, MAX_ROWS))
    return [(i, min(per, n - i)) for i in range(0, n, per)]


def igemm_split(rows, n_out, k_steps):
    """Split-K factor of one transoar_conv3d_igemm launch: 128-row tiles, 64 output channels wide up to 64 and 128 above."""
    bn = 64 if n_out <= 64 else 128
    tiles = ((rows + 127) // 128) * ((n_out + bn - 1) // bn)
    if tiles >= SPLIT_BELOW_TILES:
        return 1
    return max(1, min((SPLIT_BELOW_TILES + tiles - 1) // tiles, k_steps // 4, 16))


def igemm_ranges(n, rows_per_sample, n_in, n_out, taps, what):
    """((first, count, split), ...): the launches of an implicit-GEMM forward or data gradient that contracts `taps` taps
    of n_in channels into n_out; every batch range has the split of its own row count."""
    k_steps = (taps * n_in + 63) // 64
    return tuple((i, c, igemm_split(c * rows_per_sample, n_out, k_steps)) for i, c in batch_ranges(n, rows_per_sample, what))


def dgrad_gemm(n, cin, cout, d, h, w, stride, knobs=KNOBS, general=False):
    """-> (route, ranges) of conv_gemm's data gradient of dx (n, cin, d, h, w); general: not the halo-tile kernel."""
    if stride == 1:
        return "igemm_s1", igemm_ranges(n, d * h * w, cout, cin, 27, "conv_dgrad")
    if not general and knobs.dgrad_s2_halo and cin <= 32 and cout in (16, 32, 48):
        # few input channels, full-resolution dx: one workgroup computes all eight parity classes of a dx tile (HBM bound)
        return "s2_halo", ((0, n, 1),)
    # stride 2: the eight parity classes (pd, ph, pw) of the dx voxels in one launch: 1, 2, 4 or 8 taps each;
    # the split goes by the K steps of the eight-tap class
    return "s2_classes", igemm_ranges(n, d * h * w, cout, cin, 8, "conv_dgrad")


def wgrad_chunks(rows, cin, cout, taps):
    """Row chunks (workgroups per filter tile) of a transoar_conv3d_wgrad / transoar_linear_wgrad_bias launch."""
    bt = 64 if (cin <= 64 and cout <= 64) else 128
    tiles = taps * ((cout + bt - 1) // bt) * ((cin + bt - 1) // bt)
    budget = WGRAD_BLOCKS * (2 if (rows >= (1 << 20) or tiles >= 64) else 1)      # tools/tune_wgrad.py
    return max(1, min(budget // tiles, rows // 1024 if rows >= 1024 else 1))      # >= 16 K steps of 64 rows per block


def wgrad_gemm(n, cin, cout, od, oh, ow, knobs=KNOBS):
    """-> ("ring", chunks) or ("voxel_major", ((first, count, chunks), ...)) of conv_gemm's weight gradient."""
    rows = od * oh * ow
    # the LDS-ring weight gradient (conv_wgrad_ring.hpp): up to 64 channels on either side and more than 32 on at least
    # one, W-rows of dy in 64-voxel units, enough voxels to keep one persistent workgroup per CU busy
    if (knobs.wgrad_ring and cin <= 64 and cout <= 64 and max(cin, cout) > 32 and cin % 8 == 0 and cout % 8 == 0
            and ow % 64 == 0 and n * rows >= (1 << 18)):
        return "ring", WGRAD_RING_CHUNKS
    return "voxel_major", tuple((i, c, wgrad_chunks(c * rows, cin, cout, 27)) for i, c in batch_ranges(n, rows, "conv_wgrad"))


def wgrad_c1(n, cout, d, h, w, knobs=KNOBS):
    """-> (route, partial tiles) of the Cin = 1 weight gradient."""
    if knobs.c1_wgrad_tr and cout % 8 == 0 and w % 64 == 0 and w <= 256:      # coalesced loads + transposing LDS reads
        return "c1_tr", min(C1_WGRAD_TR_PARTIALS, n * d * h)
    return "c1", min(C1_WGRAD_PARTIALS, max(1, (n * d * h + 3) // 4))


def wgrad_lds(cin, cout, knobs=KNOBS):
    """-> (route, workgroups, ((co0, co_n, ci0, ci_n), ...)): one launch per block of <= 32 x 32 channels."""
    blocks = tuple((co0, min(32, cout - co0), ci0, min(32, cin - ci0)) for co0 in range(0, cout, 32) for ci0 in range(0, cin, 32))
    return ("lds_tr", LDS_WGRAD_TR_GROUPS, blocks) if knobs.wgrad_tr else ("lds", LDS_WGRAD_GROUPS, blocks)


def _stat_rows(n, d, h, w, cin, cout):
    from .conv3d import lib          # the halo-tile kernel's own coverage rule and tile counts: host arithmetic in the library
    return lib.transoar_conv3d_k3_stat_rows(n, d, h, w, cin, cout, 1)


_ENTRY = {"stats_halo": "transoar_conv3d_k3_forward_stats", "c1_halo": "transoar_conv3d_k3_forward_c1",
          "c1_padded": "transoar_conv3d_k3_forward", "direct": "transoar_conv3d_k3_forward",
          "direct_flipped": "transoar_conv3d_k3_forward", "s2_halo": "transoar_conv3d_dgrad_s2_halo",
          "c1_tr": "transoar_conv3d_c1_wgrad_tr", "c1": "transoar_conv3d_c1_wgrad",
          "lds_tr": "transoar_conv3d_k3_wgrad_tr", "lds": "transoar_conv3d_k3_wgrad_lds",
          "ring": "transoar_conv3d_wgrad_ring", "voxel_major": "transoar_conv3d_wgrad", "channels_first": "transoar_conv3d_k3_wgrad"}
_IGEMM = ("igemm", "igemm_s1", "s2_classes")


class ConvPlan(NamedTuple):
    stride: int
    fwd: str                 # stats_halo | c1_halo | c1_padded | direct | igemm
    fwd_ranges: tuple        # ((first, count, split), ...)
    stat_rows: int           # stats_halo: rows of the statistics' partial sums
    dgrad: str               # igemm_s1 | s2_halo | s2_classes | direct_flipped
    dgrad_ranges: tuple      # ((first, count, split), ...)
    wgrad: str               # c1_tr | c1 | lds_tr | lds | ring | voxel_major | channels_first
    wgrad_parts: int         # c1*: partial tiles; lds*: workgroups; ring: chunks
    wgrad_blocks: tuple      # lds*: ((co0, co_n, ci0, ci_n), ...)
    wgrad_ranges: tuple      # voxel_major: ((first, count, chunks), ...)

    @property
    def packs(self):
        """Does the layer want the (wk, wkt) filter packs of conv_gemm.PackPlan?"""
        return self.fwd == "igemm"

    def launches(self, direction):
        """The C entry points one call issues through _native.launch, in order; direction: fwd | dgrad | wgrad."""
        route = getattr(self, direction)
        if route in _IGEMM:
            names = []
            for _, _, split in (self.fwd_ranges if direction == "fwd" else self.dgrad_ranges):
                names += ["transoar_conv3d_igemm", "transoar_conv3d_finish"] if split > 1 else ["transoar_conv3d_igemm"]
            return names
        if direction == "wgrad":
            return [_ENTRY[route]] * max(1, len(self.wgrad_blocks), len(self.wgrad_ranges))
        return [_ENTRY[route]]


@functools.lru_cache(maxsize=None)
def plan_conv(n, cin, cout, d, h, w, stride, want_stats=False, knobs=KNOBS):
    """The kernels of a 3x3x3, padding-1 convolution of x (n, cin, d, h, w) bf16 into cout channels, or None when no
    hand-written kernel takes the shape."""
    if stride not in (1, 2) or not (cin % 8 == 0 or (cin == 1 and stride == 1 and cout <= 64)):
        return None
    if cout % 8 != 0 or (w // stride) % 8 != 0 or (stride == 2 and (d % 2 or h % 2 or w % 2)):
        return None
    od, oh, ow = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
    gemm = use_gemm(cin, cout, stride)
    whole = ((0, n, 1),)

    # the caller normalises the output next (EncoderCnnBlock): statistics in the conv epilogue where the halo-tile
    # kernel takes the layer
    stat_rows = _stat_rows(n, d, h, w, cin, cout) if want_stats and knobs.conv_stats and stride == 1 and not gemm else 0
    if stat_rows:
        fwd, fwd_ranges = "stats_halo", whole
    elif cin == 1:
        # one input channel: through the MFMA implicit GEMM with the channel axis zero-padded to 8 (K = 27 taps x 8); the
        # scalar stencil kernel (transoar_conv3d_c1_forward) is VALU-bound at a seventh of this speed -- 1.6 ms vs
        # 0.35 ms on the 2x160x160x256 volume.  From 2^16 voxels the LDS halo-tile kernel reads the one-channel volume
        # itself (zero-extends while staging).
        fwd, fwd_ranges = ("c1_halo" if cout <= 32 and d * h * w >= (1 << 16) else "c1_padded"), whole
    elif gemm:
        # 48 channels and up (and the strided 24 -> 48 layer): LDS-tiled implicit GEMM (csrc/conv_gemm.hip)
        fwd, fwd_ranges = "igemm", igemm_ranges(n, od * oh * ow, cin, cout, 27, "conv_forward")
    else:
        fwd, fwd_ranges = "direct", whole

    # data gradient off the implicit GEMM = convolution of dy with the flipped, in/out-swapped filter; always stride 1:
    # use_gemm takes every strided layer this function admits
    dgrad, dgrad_ranges = dgrad_gemm(n, cin, cout, d, h, w, stride, knobs) if gemm else ("direct_flipped", whole)

    parts, blocks, wgrad_ranges = 0, (), ()
    if stride == 1 and cin == 1 and cout <= 32 and w % 16 == 0:
        wgrad, parts = wgrad_c1(n, cout, d, h, w, knobs)      # one input channel: MFMA over voxel chunks
    elif (stride == 1 and cin % 8 == 0 and cin <= 64 and cout <= 64 and w % 64 == 0
          and (max(cin, cout) <= 32 or n * od * oh * ow >= (1 << 21))):
        wgrad, parts, blocks = wgrad_lds(cin, cout, knobs)      # few channels, 10^7 voxels: LDS-transposed MFMA
    elif cin % 8 == 0:
        # voxel-major GEMM with transposing LDS reads (batch ranges above 2^21 rows), or its LDS-ring version
        wgrad, detail = wgrad_gemm(n, cin, cout, od, oh, ow, knobs)
        parts, wgrad_ranges = (detail, ()) if wgrad == "ring" else (0, detail)
    else:
        wgrad = "channels_first"      # channels-first shifted copies: any channel count (raises on what it cannot address)
    return ConvPlan(stride, fwd, fwd_ranges, stat_rows, dgrad, dgrad_ranges, wgrad, parts, blocks, wgrad_ranges)
