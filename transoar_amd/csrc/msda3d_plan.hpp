// MSDeformAttn-3D: which kernels run for a shape, dtypes and flags.  Pure host arithmetic -- no HIP call and no kernel
// in here; the kernel headers are included for the structs the kernels read (BrickOrder, CoarseLevels) and their tile
// constants.  msda3d.hip obtains a plan first, returns a non-OK status before its first HIP call, then switches on
// the kernel codes (TRANSOAR_FWD_* / _BWD_QUERY_* / _BWD_VALUE_* of the public header) and launches;
// transoar_msda3d_plan hands the same codes to the caller.
#pragma once
#include "../../include/transoar_msda3d.h"
#include "msda3d_cells_mma.hpp"   // kCmCellChunk; msda3d_tile.hpp (kTileC, kCellChunk, CoarseLevels); msda3d_scatter.hpp (kScanTile)
#include "msda3d_pcm.hpp"         // kPcmLevels; msda3d_mma.hpp (kMmaLevels); msda3d_common.hpp (BrickOrder, kBrick*)

namespace transoar {

struct Dims { int N, S, M, C, L, Lq, P; };

static inline size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// Can the vector kernels run this problem?  (32-bit byte offsets into value, 32-bit bin / point indices.)
// -> log2 of the lanes per value row (rows of 128 / 256 / 512 bytes), or -1: the generic kernels.
static inline int vec_lpv(const Dims& d, int elt, unsigned flags) {
  if (flags & TRANSOAR_MSDA3D_FORCE_GENERIC) return -1;
  const long value_bytes = static_cast<long>(d.N) * d.S * d.M * d.C * elt;
  const long n_points = static_cast<long>(d.N) * d.Lq * d.M * d.L * d.P;
  const long n_bins = static_cast<long>(d.N) * d.M * 8 * d.S;
  if (value_bytes >= 0xfffffff0L || n_points >= (1L << 31) - 1 || n_bins >= (1L << 31) - 1) return -1;
  // row index and row pitch go through the 24-bit multiplier
  if (static_cast<long>(d.N) * d.S >= (1L << 24) || static_cast<long>(d.M) * d.C * elt >= (1L << 24)) return -1;
  if (n_points * 32 >= 0xfffffff0L) return -1;   // record array addressed with 32-bit byte offsets
  if (static_cast<long>(d.N) * d.Lq * d.M >= (1L << 24) ||
      static_cast<long>(d.N) * d.Lq * d.M * d.C * elt >= 0x7ffffff0L) return -1;
  const long row_bytes = static_cast<long>(d.C) * elt;
  return row_bytes == 128 ? 3 : row_bytes == 256 ? 4 : row_bytes == 512 ? 5 : -1;
}

// Brick schedule from host-side level shapes (NULL -> linear order).  `rows` is what the
// kernel's row index ranges over (S for voxel rows; Lq for queries, usable only when Lq == S,
// i.e. the queries ARE the pyramid's voxels as in the refine block's self-attention).
static BrickOrder make_order(const int64_t* host_shapes, const Dims& d, int rows) {
  BrickOrder o{};
  if (!host_shapes || rows != d.S) return o;
  long start = 0, pad = 0;
  for (int l = 0; l < d.L; ++l) {
    const long D = host_shapes[3 * l], H = host_shapes[3 * l + 1], W = host_shapes[3 * l + 2];
    if (D <= 0 || H <= 0 || W <= 0) return BrickOrder{};
    o.D[l] = static_cast<int>(D); o.H[l] = static_cast<int>(H); o.W[l] = static_cast<int>(W);
    o.start[l] = static_cast<int>(start);
    o.nbh[l] = static_cast<int>((H + kBrickH - 1) / kBrickH);
    o.nbw[l] = static_cast<int>((W + kBrickW - 1) / kBrickW);
    o.pad_start[l] = static_cast<int>(pad);
    pad += ((D + kBrickD - 1) / kBrickD) * o.nbh[l] * o.nbw[l] * kBrickSlots;
    start += D * H * W;
  }
  if (start != d.S || pad * d.N * d.M >= (1L << 31)) return BrickOrder{};
  o.pad_start[d.L] = static_cast<int>(pad);
  o.L = d.L;
  o.enabled = 1;
  return o;
}
static inline long order_units(const BrickOrder& o, const Dims& d, int rows) {
  return static_cast<long>(d.N) * d.M * (o.enabled ? o.pad_start[o.L] : rows);
}

// ---- the eligibility fragments, each written once --------------------------------------------------------------
// LDS-tiled (brick) kernels: rows walked in host-known bricks, 16-bit storage (an fp32 box of the finest level does
// not fit the 48 KiB tile), 64 channels per head, 4 points per level -- the refine block's configuration
static inline bool brick_form(const BrickOrder& o, const Dims& d, int value_size, unsigned flags) {
  return o.enabled && value_size == 2 && d.C == 64 && d.P == 4 && !(flags & TRANSOAR_MSDA3D_NO_BRICK);
}
// matrix-core kernels on top of that: level loops unrolled kMmaLevels times, 10-bit packed voxel coordinates
static_assert(kPcmLevels == kMmaLevels, "the point-column gather unrolls the same number of levels");
static inline bool small(const BrickOrder& o, const Dims& d) {
  bool ok = d.L <= kMmaLevels;
  for (int l = 0; ok && l < d.L; ++l) ok = o.D[l] <= 1000 && o.H[l] <= 1000 && o.W[l] <= 1000;
  return ok;
}
static inline bool mma_form(const BrickOrder& o, const Dims& d, int value_size, unsigned flags) {
  return brick_form(o, d, value_size, flags) && small(o, d) && !(flags & TRANSOAR_MSDA3D_NO_MMA);
}
// point-column gather (msda3d_pcm.hpp) on top of that: every buffer addressable with 32-bit byte offsets
static inline bool pcm_ok(const BrickOrder& o, const Dims& d) {
  const long n_pts = static_cast<long>(d.N) * d.Lq * d.M * d.L * d.P;
  const long n_wave = static_cast<long>(d.N) * (o.pad_start[o.L] >> 7) * d.M * 16;
  const long vbytes = static_cast<long>(d.N) * d.S * d.M * d.C * 2;
  return d.Lq == d.S && n_pts * 12 < 0xfffffff0L && n_wave < (1L << 31) - 8 && vbytes < 0xffffff00L;
}
// grad_proj (transoar_msda3d_backward_proj): the head's backward in the tail of the matrix-core query kernel, which
// holds the L * P = 16 points of a (query, head) in one lane group; fp32 locations as the head kernel writes them
static inline bool proj_form(const Dims& d, int value_size, int loc_size) {
  return value_size == 2 && loc_size == 4 && d.L * d.P == 16;
}

// ---- forward ---------------------------------------------------------------------------------------------------
struct FwdPlan {
  int kernel, lg;                    // TRANSOAR_FWD_*; vec: log2 lanes per value row
  BrickOrder order;                  // over the queries (enabled only when Lq == S)
  unsigned vbytes;                   // bytes of value
  long n_items, n_units, n_blocks;   // (batch, query, head) items; the same in brick order, padded; vec workgroups
  long n_waves;                      // brick: workgroups; mma / pcm: waves; q16: units (bricks x heads x 1 / 4 / 16 / 8)
  long n_pts;                        // sampling points
};

static FwdPlan plan_fwd(const Dims& d, int value_size, int loc_size, const int64_t* host_shapes, unsigned flags) {
  FwdPlan p{};
  p.lg = vec_lpv(d, value_size, flags);
  p.order = make_order(host_shapes, d, d.Lq);
  p.vbytes = static_cast<unsigned>(static_cast<long>(d.N) * d.S * d.M * d.C * value_size);
  p.n_items = static_cast<long>(d.N) * d.Lq * d.M;
  p.n_units = order_units(p.order, d, d.Lq);
  p.n_blocks = ((p.order.enabled ? p.n_units : p.n_items) + kWavesPerBlock - 1) / kWavesPerBlock;
  p.n_pts = p.n_items * d.L * d.P;
  if (p.lg < 0) p.kernel = TRANSOAR_FWD_GENERIC;
  else if (!brick_form(p.order, d, value_size, flags)) p.kernel = TRANSOAR_FWD_VEC;
  else if (!mma_form(p.order, d, value_size, flags)) p.kernel = TRANSOAR_FWD_BRICK;
  else if (loc_size != 4 || !pcm_ok(p.order, d) || (flags & TRANSOAR_MSDA3D_MMA_Q32)) p.kernel = TRANSOAR_FWD_MMA;
  // 16 queries per wave (msda3d_q16.hpp): measured SLOWER than the 8-query kernel; kept behind
  // its flag as the carving's speed-of-light probe, parity-tested
  else p.kernel = (flags & TRANSOAR_MSDA3D_Q16) ? TRANSOAR_FWD_Q16 : TRANSOAR_FWD_PCM;
  const long per_brick = p.kernel == TRANSOAR_FWD_PCM ? 16 : p.kernel == TRANSOAR_FWD_Q16 ? 8 : p.kernel == TRANSOAR_FWD_MMA ? 4 : 1;
  p.n_waves = static_cast<long>(d.N) * (p.order.pad_start[p.order.L] >> 7) * d.M * per_brick;
  return p;
}

// ---- backward --------------------------------------------------------------------------------------------------
struct BwdWorkspace {
  size_t count, tile_sums, rank, rec_item, recs, coarse, det_keys, det_alt, det_temp, det_temp_bytes, total;
  long n_bins, n_points, n_scan, n_tiles;
};

static BwdWorkspace bwd_workspace(const Dims& d, size_t acc_size, unsigned flags) {
  BwdWorkspace w;
  w.n_points = static_cast<long>(d.N) * d.Lq * d.M * d.L * d.P;
  w.n_bins = static_cast<long>(d.N) * d.M * 8 * d.S;   // (D+1)(H+1)(W+1) <= 8*D*H*W
  w.n_scan = w.n_bins + 1;
  w.n_tiles = (w.n_scan + kScanTile - 1) / kScanTile;
  size_t off = 0;
  w.count = off;     off += align16(sizeof(int) * w.n_scan);
  w.tile_sums = off; off += align16(sizeof(int) * w.n_tiles);
  w.rank = off;      off += align16(sizeof(int) * w.n_points);
  w.rec_item = off;  off += align16(sizeof(int) * w.n_points);
  w.recs = off;      off += align16(8 * acc_size * w.n_points);   // PointW8 (tile path) or PointRec
  w.coarse = off;    off += align16(sizeof(float) * static_cast<size_t>(d.N) * d.S * d.M * d.C);   // fp32 rows of the coarse levels
  w.det_keys = w.det_alt = w.det_temp = off;
  w.det_temp_bytes = 0;
  if (flags & TRANSOAR_MSDA3D_DETERMINISTIC) {      // two key buffers + the radix sort's scratch (histograms: a bound, checked at run time)
    w.det_keys = off;  off += align16(sizeof(unsigned long long) * w.n_points);
    w.det_alt = off;   off += align16(sizeof(unsigned long long) * w.n_points);
    w.det_temp_bytes = align16((size_t(32) << 20) + static_cast<size_t>(w.n_points));
    w.det_temp = off;  off += w.det_temp_bytes;
  }
  w.total = off;
  return w;
}

constexpr long kCoarsePointsPerVoxel = 32;   // measured: 128 -> 32 moves level 1 of the flagship pyramid to the chunked walk (2.00 -> 1.90 ms serial)

struct BwdPlan {
  int status;                   // TRANSOAR_OK, or TRANSOAR_ERR_MODE: nothing may be launched
  int query, value, lg;         // TRANSOAR_BWD_QUERY_*, TRANSOAR_BWD_VALUE_*
  bool sorted_by_query;         // query is _MMA / _MMA_DET: it has counted, scanned and written the sorted records
  bool fold_count;              // the query kernel bins the points; else msda3d_cell_count after it
  bool pull_head_major;         // _VALUE_PULL walks the bricks head by head (r_order.enabled == 2)
  long cells_per_slab, n_scan, n_tiles;      // cells of one (batch, head) slab; entries of count[] in use and their scan tiles
  BrickOrder q_order, r_order;               // over the queries / over the voxel rows
  long n_items, q_units, q_blocks, q_waves;  // query work: items, ordered units, vec workgroups, brick workgroups (x 4: mma waves)
  size_t value_elems;
  unsigned vbytes;
  CoarseLevels coarse;          // tile walks: levels first..L-1 go to the chunked cell walk
  int fine_bricks;              // tile walks: bricks of the levels below coarse.first
  BwdWorkspace ws;              // scratch layout; ws.total is what transoar_msda3d_backward_workspace_bytes returns
};

// ws (and so the workspace size) is filled whatever the status: it does not depend on host_shapes.
static BwdPlan plan_bwd(const Dims& d, int value_size, int loc_size, const int64_t* host_shapes, unsigned flags,
                        bool want_grad_proj) {
  BwdPlan p{};
  const bool det = (flags & TRANSOAR_MSDA3D_DETERMINISTIC) != 0;
  const size_t acc_size = value_size == 8 ? 8 : 4;      // sizeof(Elem<VT>::acc)
  p.lg = vec_lpv(d, value_size, flags);
  p.n_items = static_cast<long>(d.N) * d.Lq * d.M;
  p.value_elems = static_cast<size_t>(d.N) * d.S * d.M * d.C;
  p.vbytes = static_cast<unsigned>(p.value_elems * value_size);
  p.coarse = CoarseLevels{d.L, 0, d.S, 0, 0};
  if (p.lg < 0) {
    // scatter with fp atomics into a zeroed accumulator (fp32 for 16-bit storage: that is the workspace): neither
    // bit-stable nor able to write grad_proj
    p.query = TRANSOAR_BWD_QUERY_GENERIC;
    p.value = TRANSOAR_BWD_VALUE_GENERIC;
    p.ws.total = value_size == 2 ? align16(sizeof(float) * p.value_elems) : 0;
    p.status = (det || want_grad_proj) ? TRANSOAR_ERR_MODE : TRANSOAR_OK;
    return p;
  }
  p.ws = bwd_workspace(d, acc_size, flags);
  p.q_order = make_order(host_shapes, d, d.Lq);
  p.r_order = make_order(host_shapes, d, d.S);
  p.q_units = order_units(p.q_order, d, d.Lq);
  p.q_blocks = (p.q_units + kWavesPerBlock - 1) / kWavesPerBlock;
  p.q_waves = static_cast<long>(d.N) * (p.q_order.pad_start[p.q_order.L] >> 7) * d.M;
  // cells per (batch, head) slab: needs the level shapes on the host; without them the binning
  // runs as its own kernel (msda3d_cell_count) after the gather
  if (host_shapes)
    for (int l = 0; l < d.L; ++l)
      p.cells_per_slab += (host_shapes[3 * l] + 1) * (host_shapes[3 * l + 1] + 1) * (host_shapes[3 * l + 2] + 1);
  const long cells = p.cells_per_slab * d.N * d.M;
  p.fold_count = host_shapes != nullptr && cells <= p.ws.n_bins;

  // 1. grad_loc / grad_attn.  The matrix-core chain (count, scan, one kernel that also writes every point's record at
  // its sorted position) is the only one with a deterministic order (needs one more scanned entry; the sort takes the
  // point count as an int) and the only one that writes grad_proj: no silent fall-back for either.
  p.sorted_by_query = p.fold_count && mma_form(p.q_order, d, value_size, flags);
  if (det && !(p.sorted_by_query && cells + 2 <= p.ws.n_scan && p.ws.n_points < (1L << 31))) p.status = TRANSOAR_ERR_MODE;
  if (want_grad_proj && !(p.sorted_by_query && proj_form(d, value_size, loc_size))) p.status = TRANSOAR_ERR_MODE;
  if (p.status != TRANSOAR_OK) return p;
  p.query = p.sorted_by_query ? (det ? TRANSOAR_BWD_QUERY_MMA_DET : TRANSOAR_BWD_QUERY_MMA)
            : (p.fold_count && brick_form(p.q_order, d, value_size, flags)) ? TRANSOAR_BWD_QUERY_BRICK : TRANSOAR_BWD_QUERY_VEC;
  // entries of the count / offset array in use: one per cell + the end of the last run (the upper bound n_bins + 1 =
  // 8 S N M + 1 without host shapes: zeroing and scanning it was 45 MB four times over at the flagship size);
  // deterministic mode reads the walks' offsets one entry further on
  p.n_scan = p.fold_count ? cells + 1 + (det ? 1 : 0) : p.ws.n_scan;
  p.n_tiles = (p.n_scan + kScanTile - 1) / kScanTile;

  // 2. grad_value.  Brick-owner schedule (fp32 LDS tile per 4x4x8 brick) for fp32 accumulation and kTileC channels;
  // 16-bit storage walks 16-byte records on the matrix cores, fp32 storage 8-weight records.
  if (acc_size == 4 && p.r_order.enabled && p.fold_count && d.C == kTileC && !(flags & TRANSOAR_MSDA3D_NO_BRICK)) {
    const bool mma = value_size == 2 && !(flags & TRANSOAR_MSDA3D_NO_MMA);
    p.value = mma ? TRANSOAR_BWD_VALUE_TILE_MMA : TRANSOAR_BWD_VALUE_TILE_W8;
    // levels whose voxels receive >= kCoarsePointsPerVoxel points each go to the chunked walk
    // (deterministic mode: no coarse level -- their walk flushes with fp32 atomics)
    p.coarse.cell_start = static_cast<int>(p.cells_per_slab);
    for (int l = d.L - 1; l >= 0 && !det; --l) {
      const long vox = host_shapes[3 * l] * host_shapes[3 * l + 1] * host_shapes[3 * l + 2];
      if (static_cast<long>(d.Lq) * d.P < kCoarsePointsPerVoxel * vox) break;
      p.coarse.first = l;
      p.coarse.cell_start -= static_cast<int>((host_shapes[3 * l] + 1) * (host_shapes[3 * l + 1] + 1) * (host_shapes[3 * l + 2] + 1));
      p.coarse.row_start = p.r_order.start[l];
    }
    p.coarse.rows = d.S - p.coarse.row_start;
    const int cell_chunk = mma ? kCmCellChunk : kCellChunk;
    p.coarse.chunks_per_slab = static_cast<int>((static_cast<long>(d.Lq) * d.P * (d.L - p.coarse.first) + cell_chunk - 1) / cell_chunk) + 1;
    p.fine_bricks = p.r_order.pad_start[p.coarse.first] >> 7;
  } else {
    p.value = TRANSOAR_BWD_VALUE_PULL;
    p.pull_head_major = p.r_order.enabled && (flags & TRANSOAR_MSDA3D_PULL_HEAD_MAJOR);
    if (p.pull_head_major) p.r_order.enabled = 2;
  }
  // The matrix-core query kernels have already written 16-byte records at their sorted positions, which only the
  // matrix-core tile walk reads.  mma_form on q_order (Lq == S, so r_order is the same order) implies that walk.
  if (p.sorted_by_query && p.value != TRANSOAR_BWD_VALUE_TILE_MMA) p.status = TRANSOAR_ERR_MODE;
  return p;
}

}  // namespace transoar
