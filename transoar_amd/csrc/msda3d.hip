// MSDeformAttn-3D for MI355X (gfx950): the C ABI of include/transoar_msda3d.h
// and the host-side dispatch onto the kernels in
//   msda3d_gather.hpp   forward + grad_loc/grad_attn (query-stationary gathers)
//   msda3d_scatter.hpp  grad_value (cell sort + voxel-stationary pull, no atomics)
//   msda3d_generic.hpp  any-C / fp64 correctness kernels
// Which of them run for a shape and flags is decided in msda3d_plan.hpp (host only).
//
// What is computed is fixed by the reference (semantics: SURVEY.md appendix A;
// ops/src/cuda/ms_deform_im2col_cuda.cuh:31-114, 116-241, 370-439).  How is
// not: see the kernel headers.  Bound: HBM/L2 bandwidth (18 flop per gathered
// byte); no MFMA in here.
#include <algorithm>
#include <cstring>

#include "../../include/transoar_msda3d.h"
#include "msda3d_common.hpp"
#include "msda3d_brick.hpp"
#include "msda3d_mma.hpp"
#include "msda3d_pcm.hpp"
#include "msda3d_q16.hpp"
#include "msda3d_tile.hpp"
#include "msda3d_cells_mma.hpp"
#include "msda3d_gather.hpp"
#include "msda3d_generic.hpp"
#include "msda3d_scatter.hpp"
#include "msda3d_plan.hpp"

#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace transoar {

// ---- optional per-kernel timing with HIP events on the launch stream -------
// bench.py turns this on for the timed region: every kernel launched by the
// two entry points is bracketed by an event pair recorded on `stream`; the
// pairs are resolved later by transoar_msda3d_profile_read (which synchronises
// on them).  Off by default: zero cost.
struct ProfPair { hipEvent_t beg, end; int kind; };
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfPair> g_prof_live;   // recorded, not yet read
static std::vector<ProfPair> g_prof_free;   // reusable event pairs

struct ProfScope {
  hipStream_t st;
  ProfPair pair;
  bool on;
  ProfScope(int kind, hipStream_t s) : st(s), on(false) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_on) return;
    if (!g_prof_free.empty()) {
      pair = g_prof_free.back();
      g_prof_free.pop_back();
    } else if (hipEventCreate(&pair.beg) != hipSuccess || hipEventCreate(&pair.end) != hipSuccess) {
      return;
    }
    pair.kind = kind;
    on = hipEventRecord(pair.beg, st) == hipSuccess;
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(pair.end, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_live.push_back(pair);
  }
};

// Side stream for the coarse-level walk of grad_value: it and the fine-level tile walk are both
// latency-bound and independent until the final row store, so they are forked onto two streams
// (event fork / join on the caller's stream; captured as two branches under HIP graph capture).
// One pair per device, created on first use (an eager call, before any capture).
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool ok = false;
};
static SideStream* side_stream() {
  static std::mutex mu;
  static SideStream per_device[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  SideStream& s = per_device[dev];
  if (!s.ok && s.stream == nullptr) {
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&s.join, hipEventDisableTiming) == hipSuccess)
      s.ok = true;
  }
  return s.ok ? &s : nullptr;
}

// zero-fill as a kernel launch (16 bytes per thread; n16 = number of 16-byte pieces)
__global__ __launch_bounds__(256) void msda3d_zero16(u32x4* __restrict__ p, long n16) {
  const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n16) p[i] = u32x4{0u, 0u, 0u, 0u};
}
static inline hipError_t zero_async(void* p, size_t bytes, hipStream_t st) {
  if (getenv("TRANSOAR_MSDA_MEMSET_NODE")) return hipMemsetAsync(p, 0, bytes, st);
  const long n16 = static_cast<long>((bytes + 15) / 16);           // every region is 16-byte padded
  hipLaunchKernelGGL(msda3d_zero16, dim3(static_cast<unsigned>((n16 + 255) / 256)), dim3(256), 0, st,
                     static_cast<u32x4*>(p), n16);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// host dispatch: WHICH kernels run is decided in msda3d_plan.hpp; below, a plan is obtained and launched
// ---------------------------------------------------------------------------
int sort_keys64(unsigned long long* keys, unsigned long long* alt, long n, int end_bit, void* temp, size_t* temp_bytes,
                unsigned long long** sorted, hipStream_t st);          // msda3d_sort.hip

// Launch constants of the brick-scheduled kernels (BrickOrder: ~300 bytes; CoarseLevels) live in device memory and
// the kernels read them through a pointer: kernel arguments stay a handful of scalars and pointers, which is what
// replays correctly from a captured HIP graph with ROCm's graph packet capture (large by-value kernel arguments
// are the suspect of the corrupted replays of DESIGN.md section 8).  One immutable copy per distinct content and
// device, made on first use -- a synchronous hipMalloc + hipMemcpy, so first use must be an eager call (the
// training step always runs eagerly before it is captured); returns nullptr if that is not possible.
static const void* device_const(const void* host, size_t bytes, hipStream_t st) {
  static std::mutex mu;
  static std::map<std::pair<int, std::string>, void*> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::pair<int, std::string> key(dev, std::string(static_cast<const char*>(host), bytes));
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  // not cached yet: making the copy needs hipMalloc + a synchronous hipMemcpy, neither of which may run while `st`
  // is being captured (in global capture mode the hipMalloc alone invalidates the capture): refuse instead
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
  if (cache.size() >= 256) return nullptr;            // bounded: a few entries per (device, pyramid shape) are expected
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  if (hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    return nullptr;
  }
  cache[key] = p;
  return p;
}
template <typename T> static const T* device_const(const T& v, hipStream_t st) {
  return static_cast<const T*>(device_const(&v, sizeof(T), st));
}

static float host_bf16_round(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  memcpy(&x, &u, 4);
  return x;
}
static PcmConst make_pcm_const(const BrickOrder& order) {
  PcmConst c;
  memset(&c, 0, sizeof(c));
  c.order = order;
  for (int l = 0; l < 4; ++l) {
    const int ls = l < order.L ? l : 0;
    c.fD[l] = static_cast<float>(order.D[ls]); c.fH[l] = static_cast<float>(order.H[ls]); c.fW[l] = static_cast<float>(order.W[ls]);
    c.dD[l] = host_bf16_round(c.fD[l]); c.dH[l] = host_bf16_round(c.fH[l]); c.dW[l] = host_bf16_round(c.fW[l]);
  }
  return c;
}

// Launch constants of msda3d_fwd_q16: the point-column constants + the reciprocals of its unit decode
static Q16Const make_q16_const(const BrickOrder& order, int M) {
  Q16Const c;
  memset(&c, 0, sizeof(c));
  c.pc = make_pcm_const(order);
  auto mg = [](long d) -> unsigned long long { return (1ull << 40) / static_cast<unsigned long long>(d > 0 ? d : 1) + 1ull; };
  c.mg_M = mg(M);
  c.mg_bricks = mg(order.pad_start[order.L] >> 7);
  for (int l = 0; l < 4; ++l) {
    c.mg_nbw[l] = mg(l < order.L ? order.nbw[l] : 1);
    c.mg_nbh[l] = mg(l < order.L ? order.nbh[l] : 1);
  }
  return c;
}
// LAUNCH(3 | 4 | 5): the vector kernels are templated on log2 of the lanes per value row
#define TRANSOAR_BY_LG(LG, LAUNCH) do { if (LG == 3) LAUNCH(3); else if (LG == 4) LAUNCH(4); else LAUNCH(5); } while (0)
static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

template <typename VT, typename LT>
static int launch_fwd(const void* value, const int64_t* shapes, const int64_t* lsi,
                      const void* loc, const void* attn, void* out, const Dims& d,
                      const int64_t* host_shapes, unsigned flags, hipStream_t st) {
  const FwdPlan p = plan_fwd(d, sizeof(VT), sizeof(LT), host_shapes, flags);
  const BrickOrder& order = p.order;
  const dim3 block(64 * kWavesPerBlock);
  const dim3 wgrid(static_cast<unsigned>(((p.n_waves + 7) / 8) * 8));      // brick / mma / pcm: one workgroup or wave per p.n_waves
  auto v = static_cast<const VT*>(value);
  auto lo = static_cast<const LT*>(loc);
  auto at = static_cast<const LT*>(attn);
  auto o = static_cast<VT*>(out);
  ProfScope prof(p.kernel == TRANSOAR_FWD_GENERIC ? TRANSOAR_PROF_FWD_GENERIC : TRANSOAR_PROF_FWD, st);
  switch (p.kernel) {
    case TRANSOAR_FWD_GENERIC:
      hipLaunchKernelGGL((msda3d_fwd_generic<VT, LT>), dim3((p.n_items + kWavesPerBlock - 1) / kWavesPerBlock),
                         block, 0, st, v, shapes, lsi, lo, at, o, d.S, d.M, d.C, d.L, d.Lq, d.P, p.n_items);
      break;
    case TRANSOAR_FWD_VEC: {
      const dim3 grid(((p.n_blocks + 7) / 8) * 8);
#define TRANSOAR_FWD(LG)                                                                      \
  hipLaunchKernelGGL((msda3d_fwd_vec<VT, LT, LG>), grid, block, 0, st, v, shapes, lsi, lo, at, \
                     o, d.S, d.M, d.C, d.L, d.Lq, d.P, p.vbytes, p.n_units, p.n_blocks, order)
      TRANSOAR_BY_LG(p.lg, TRANSOAR_FWD);
#undef TRANSOAR_FWD
      break;
    }
    case TRANSOAR_FWD_BRICK:       // LDS-tiled, per corner: one workgroup per brick and head
      hipLaunchKernelGGL((msda3d_fwd_brick<VT, LT, 4, 64>), wgrid, dim3(kBrickThreads), kTileBytes, st, v, lo, at, o,
                         d.S, d.M, d.L, p.n_waves, order);
      break;
    case TRANSOAR_FWD_MMA:         // matrix-core gather: one wave per 32 queries (2x4x4 sub-brick) and head
      if constexpr (sizeof(VT) == 2) {
        const BrickOrder* order_d = device_const(order, st);
        if (order_d == nullptr) return TRANSOAR_ERR_CONST;
        hipLaunchKernelGGL((msda3d_fwd_mma<VT, LT>), wgrid, dim3(64), 0, st, v, lo, at, o, d.S, d.M, d.L, p.vbytes,
                           p.n_waves, order_d);
      }
      break;
    case TRANSOAR_FWD_PCM:         // point-column form (msda3d_pcm.hpp): one wave per 8 queries (2x2x2 sub-brick) and head
      if constexpr (sizeof(VT) == 2 && sizeof(LT) == 4) {
        const PcmConst* cst = device_const(make_pcm_const(order), st);
        if (cst == nullptr) return TRANSOAR_ERR_CONST;
        hipLaunchKernelGGL((msda3d_fwd_pcm<VT, false>), wgrid, dim3(64), 0, st, v, lo, at, nullptr, nullptr, 0u, o,
                           d.S, d.M, d.L, p.vbytes, static_cast<unsigned>(p.n_pts * 12), static_cast<unsigned>(p.n_pts * 4),
                           static_cast<unsigned>(p.n_waves), cst);
      }
      break;
    case TRANSOAR_FWD_Q16:         // 16 queries per wave (msda3d_q16.hpp); p.n_waves counts its units, `upw` of them per wave
      if constexpr (sizeof(VT) == 2 && sizeof(LT) == 4) {
        static const int upw_env = env_int("TRANSOAR_MSDA3D_Q16_UPW", 4), probe = env_int("TRANSOAR_MSDA3D_Q16_PROBE", 0);
        const unsigned upw = static_cast<unsigned>(upw_env < 1 ? 1 : (upw_env > 64 ? 64 : upw_env));
        const long n_waves = (p.n_waves + upw - 1) / upw;
        const Q16Const* cst = device_const(make_q16_const(order, d.M), st);
        if (cst == nullptr) return TRANSOAR_ERR_CONST;
        const dim3 grid(static_cast<unsigned>(((n_waves + 7) / 8) * 8));
#define TRANSOAR_Q16(PROBE)                                                                                             \
  hipLaunchKernelGGL((msda3d_fwd_q16<VT, PROBE>), grid, dim3(64), 0, st, v, lo, at, o, d.S, d.M, d.L, p.vbytes,           \
                     static_cast<unsigned>(p.n_pts * 12), static_cast<unsigned>(p.n_pts * 4), static_cast<unsigned>(p.n_waves), upw, cst)
        if (probe == 1) TRANSOAR_Q16(1);
        else if (probe == 2) TRANSOAR_Q16(2);
        else if (probe == 3) TRANSOAR_Q16(3);
        else TRANSOAR_Q16(0);
#undef TRANSOAR_Q16
      }
      break;
  }
  return static_cast<int>(hipGetLastError());
}

// forward with the module's sampling head fused into the gather's prologue (msda3d_pcm.hpp, FUSED): covers a form
// exactly when the plain forward (fp32 locations, no flags) takes the point-column kernel
template <typename VT>
static int launch_fwd_fused(const void* value, const void* proj, const float* ref, long ref_rows, void* out, const Dims& d,
                            const int64_t* host_shapes, hipStream_t st) {
  const FwdPlan p = plan_fwd(d, sizeof(VT), sizeof(float), host_shapes, 0u);
  if (p.kernel != TRANSOAR_FWD_PCM) return TRANSOAR_ERR_DIM;
  if (ref_rows != d.Lq && ref_rows != static_cast<long>(d.N) * d.Lq) return TRANSOAR_ERR_DIM;
  ProfScope prof(TRANSOAR_PROF_FWD, st);
  const PcmConst* cst = device_const(make_pcm_const(p.order), st);
  if (cst == nullptr) return TRANSOAR_ERR_CONST;
  const unsigned ref_bstride = ref_rows == d.Lq ? 0u : static_cast<unsigned>(d.Lq) * d.L * 12u;
  const long proj_bytes = static_cast<long>(d.N) * d.S * 4 * d.M * d.L * d.P * 2;
  hipLaunchKernelGGL((msda3d_fwd_pcm<VT, true>), dim3(static_cast<unsigned>(((p.n_waves + 7) / 8) * 8)), dim3(64), 0, st,
                     static_cast<const VT*>(value), nullptr, nullptr, static_cast<const unsigned short*>(proj), ref, ref_bstride,
                     static_cast<VT*>(out), d.S, d.M, d.L, p.vbytes, static_cast<unsigned>(proj_bytes),
                     static_cast<unsigned>(ref_rows * d.L * 12), static_cast<unsigned>(p.n_waves), cst);
  return static_cast<int>(hipGetLastError());
}

// deterministic mode: sorted position j takes the record of the canonical slot in the low half of its key
__global__ __launch_bounds__(256) void msda3d_det_gather(const unsigned long long* __restrict__ sorted, const PointR16* __restrict__ slots,
                                                          PointR16* __restrict__ recs, long n) {
  const long j = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = sorted[j];
  if (k == ~0ull) return;
  recs[j] = slots[static_cast<unsigned>(k)];
}

#define TRANSOAR_CHECK_HIP(expr)                         \
  do {                                                   \
    const hipError_t e_ = (expr);                        \
    if (e_ != hipSuccess) return static_cast<int>(e_);   \
  } while (0)

// One backward call: the plan, typed views of the caller's buffers and of the workspace regions, and the launch of
// each stage.  run() is the whole sequence; no stage decides anything the plan has not decided.
template <typename VT, typename LT>
struct BwdLaunch {
  using A = typename Elem<VT>::acc;
  const Dims& d;
  const BwdPlan& p;
  hipStream_t st;
  char* ws;
  const int64_t *shapes, *lsi;
  const VT *v, *go;
  const LT *lo, *at;
  VT* gv;
  LT *gl, *ga;
  unsigned short* gp;      // grad_proj (transoar_msda3d_backward_proj) or nullptr
  bool fork;               // TRANSOAR_MSDA3D_FORK: the coarse walk of value_tile on the side stream
  const dim3 block{64 * kWavesPerBlock};
  const dim3 pgrid{static_cast<unsigned>((p.ws.n_points + 255) / 256)};        // one thread per sampling point
  int* count = reinterpret_cast<int*>(ws + p.ws.count);
  int* tile_sums = reinterpret_cast<int*>(ws + p.ws.tile_sums);
  int* rank = reinterpret_cast<int*>(ws + p.ws.rank);
  int* rec_item = reinterpret_cast<int*>(ws + p.ws.rec_item);

  int run() const {
    if (p.query == TRANSOAR_BWD_QUERY_GENERIC) return generic();
    TRANSOAR_CHECK_HIP(zero_async(count, sizeof(int) * p.n_scan, st));
    // 1. grad_loc / grad_attn (+ the binning pass of the point sort when folded)
    if (p.sorted_by_query) {
      if (const int rc = query_mma()) return rc;
    } else {
      ProfScope prof(TRANSOAR_PROF_BWD_QUERY, st);
      if (p.query == TRANSOAR_BWD_QUERY_BRICK) {
        if constexpr (sizeof(VT) == 2)
          hipLaunchKernelGGL((msda3d_bwd_query_brick<VT, LT, 4, 64>), dim3(((p.q_waves + 7) / 8) * 8), dim3(kBrickThreads),
                             kTileBytes, st, v, lo, at, go, gl, ga, count, rank, static_cast<int>(p.cells_per_slab), d.S, d.M,
                             d.L, p.q_waves, p.q_order);
      } else {
        const dim3 grid(((p.q_blocks + 7) / 8) * 8);
#define TRANSOAR_BWDQ(LG)                                                                   \
  hipLaunchKernelGGL((msda3d_bwd_query_vec<VT, LT, LG>), grid, block, 0, st, v, shapes, lsi, lo, \
                     at, go, gl, ga, p.fold_count ? count : nullptr, rank, static_cast<int>(p.cells_per_slab), \
                     d.S, d.M, d.C, d.L, d.Lq, d.P, p.vbytes, p.q_units, p.q_blocks, p.q_order)
        TRANSOAR_BY_LG(p.lg, TRANSOAR_BWDQ);
#undef TRANSOAR_BWDQ
      }
    }
    // 2. sort the sampling points by cell (the matrix-core chain has done all of it)
    if (!p.fold_count) {
      ProfScope prof(TRANSOAR_PROF_CELL_COUNT, st);
      hipLaunchKernelGGL((msda3d_cell_count<LT, A>), pgrid, dim3(256), 0, st, lo, at, shapes, lsi, count,
                         rank, d.M, d.L, d.Lq, d.P, p.ws.n_points);
    }
    if (!p.sorted_by_query) scan();
    // 3. grad_value rows
    return p.value == TRANSOAR_BWD_VALUE_PULL ? value_pull() : value_tile();
  }

  // scatter with fp atomics into a zeroed accumulator of type A
  int generic() const {
    ProfScope prof(TRANSOAR_PROF_BWD_GENERIC, st);
    A* acc = sizeof(VT) == 2 ? reinterpret_cast<A*>(ws) : reinterpret_cast<A*>(gv);
    TRANSOAR_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(A) * p.value_elems, st));
    hipLaunchKernelGGL((msda3d_bwd_generic<VT, LT>), dim3((p.n_items + kWavesPerBlock - 1) / kWavesPerBlock),
                       block, 0, st, v, shapes, lsi, lo, at, go, acc, gl, ga, d.S, d.M, d.C, d.L, d.Lq, d.P,
                       p.n_items);
    if (sizeof(VT) == 2) {
      const int cast_blocks = static_cast<int>(std::min<size_t>((p.value_elems + 255) / 256, 1 << 16));
      hipLaunchKernelGGL((msda3d_cast_rows<VT>), dim3(cast_blocks), dim3(256), 0, st,
                         reinterpret_cast<const float*>(acc), gv, static_cast<long>(p.value_elems));
    }
    return static_cast<int>(hipGetLastError());
  }

  void scan() const {
    ProfScope prof(TRANSOAR_PROF_SCAN, st);
    hipLaunchKernelGGL(msda3d_scan_tiles, dim3(static_cast<unsigned>(p.n_tiles)), dim3(kScanThreads), 0,
                       st, count, tile_sums, static_cast<int>(p.n_scan));
    hipLaunchKernelGGL(msda3d_scan_tile_sums, dim3(1), dim3(kScanThreads), 0, st, tile_sums,
                       static_cast<int>(p.n_tiles));
    hipLaunchKernelGGL(msda3d_scan_add, dim3(static_cast<unsigned>(p.n_tiles)), dim3(kScanThreads), 0, st,
                       count, tile_sums, static_cast<int>(p.n_scan));
  }

  // Matrix-core chain: count the points per cell (locations only), scan, then ONE kernel computes grad_loc /
  // grad_attn and writes every point's 16-byte record at its sorted position.  The counts go to count[cell + 1]:
  // after the exclusive scan that slot holds the first position of cell `cell` and serves as its cursor; when the
  // records are written it has advanced to the first position of cell + 1, i.e. count[] is the offset array the
  // grad_value walks read (offset[c], offset[c + 1]) without another pass.
  // Deterministic order (TRANSOAR_BWD_QUERY_MMA_DET): every point's record goes to its canonical slot (upper half of the record
  // region) with the key (cell << 32 | slot); a stable radix sort of the keys (skipped points keep the all-ones key and
  // end up last) and one gather put the records of a cell next to each other in slot order.  The exclusive scan of the
  // counts is left as it is (no cursor advanced): count[c + 1] is the FIRST position of cell c, i.e. the walks
  // read their (offset[c], offset[c + 1]) pairs from count + 1.
  int query_mma() const {
    if constexpr (sizeof(VT) == 2) {
      const bool det = p.query == TRANSOAR_BWD_QUERY_MMA_DET;
      const long n_wave = p.q_waves * 4, n_points = p.ws.n_points;
      const BrickOrder* order_d = device_const(p.q_order, st);
      if (order_d == nullptr) return TRANSOAR_ERR_CONST;
      const dim3 qgrid(static_cast<unsigned>(((n_wave + 7) / 8) * 8));
      {
        ProfScope prof(TRANSOAR_PROF_CELL_COUNT, st);
        hipLaunchKernelGGL((msda3d_cell_count_mma<LT>), qgrid, dim3(64), 0, st, lo, count + 1,
                           static_cast<int>(p.cells_per_slab), d.S, d.M, d.L, n_wave, order_d);
      }
      scan();
      PointR16* recs = reinterpret_cast<PointR16*>(ws + p.ws.recs);
      PointR16* slots = det ? recs + n_points : recs;
      auto keys = det ? reinterpret_cast<unsigned long long*>(ws + p.ws.det_keys) : nullptr;
      auto alt = reinterpret_cast<unsigned long long*>(ws + p.ws.det_alt);
      if (det) TRANSOAR_CHECK_HIP(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * n_points, st));
      {
        ProfScope prof(TRANSOAR_PROF_BWD_QUERY, st);
        hipLaunchKernelGGL((msda3d_bwd_query_mma<VT, LT>), qgrid, dim3(64), 0, st,
                           v, lo, at, go, gl, ga, count + 1, slots, keys,
                           static_cast<int>(p.cells_per_slab), d.S, d.M, d.L, p.vbytes, n_wave, order_d, gp);
      }
      if (!det) return TRANSOAR_OK;
      ProfScope prof(TRANSOAR_PROF_CELL_FILL, st);
      int cell_bits = 1;
      while ((p.cells_per_slab * d.N * d.M) >> cell_bits) ++cell_bits;
      size_t need = 0;
      int rc = sort_keys64(keys, alt, n_points, 32 + cell_bits, nullptr, &need, nullptr, st);
      if (rc != 0) return rc;
      if (need > p.ws.det_temp_bytes) return TRANSOAR_ERR_WORKSPACE;
      unsigned long long* sorted = nullptr;
      size_t temp_bytes = p.ws.det_temp_bytes;
      rc = sort_keys64(keys, alt, n_points, 32 + cell_bits, ws + p.ws.det_temp, &temp_bytes, &sorted, st);
      if (rc != 0) return rc;
      hipLaunchKernelGGL(msda3d_det_gather, dim3(static_cast<unsigned>((n_points + 255) / 256)), dim3(256), 0, st,
                         sorted, slots, recs, n_points);
    }
    return TRANSOAR_OK;
  }

  // brick-owner schedule: fp32 LDS tile per 4x4x8 brick for the fine levels, chunked cell walk for the coarse ones
  int value_tile() const {
    if constexpr (sizeof(A) == 4) {
      const bool mma = p.value == TRANSOAR_BWD_VALUE_TILE_MMA;
      const CoarseLevels& cl = p.coarse;
      const int cells = static_cast<int>(p.cells_per_slab), fine_bricks = p.fine_bricks, coarse_levels = d.L - cl.first;
      auto recs8 = reinterpret_cast<PointW8<float>*>(ws + p.ws.recs);
      auto recs4 = reinterpret_cast<PointR16*>(ws + p.ws.recs);       // matrix-core walks: 16 bytes with the row index inside
      if (!p.sorted_by_query) {
        ProfScope prof(TRANSOAR_PROF_CELL_FILL, st);
        if (mma)
          hipLaunchKernelGGL((msda3d_cell_fill_r16<LT>), pgrid, dim3(256), 0, st, lo, at, shapes, lsi, count, rank, recs4,
                             d.M, d.L, d.Lq, d.P, p.ws.n_points);
        else
          hipLaunchKernelGGL((msda3d_cell_fill_w8<LT, float>), pgrid, dim3(256), 0, st, lo, at, shapes, lsi, count,
                             rank, recs8, rec_item, d.M, d.L, d.Lq, d.P, p.ws.n_points);
      }
      const int* offsets = p.query == TRANSOAR_BWD_QUERY_MMA_DET ? count + 1 : count;
      const BrickOrder* r_order_d = device_const(p.r_order, st);
      const CoarseLevels* cl_d = device_const(cl, st);
      if (r_order_d == nullptr || cl_d == nullptr) return TRANSOAR_ERR_CONST;
      float* scratch = reinterpret_cast<float*>(ws + p.ws.coarse);
      const long scratch_elems = static_cast<long>(d.N) * cl.rows * d.M * kTileC;
      // opt-in (TRANSOAR_MSDA3D_FORK): 3.90 -> 3.59 ms per eager backward at the flagship, but 1.1 ms per
      // step SLOWER when the step is replayed as a HIP graph (fork/join nodes), which is how bench.py runs
      SideStream* side = (g_prof_on || !fork || coarse_levels == 0 || fine_bricks == 0) ? nullptr : side_stream();
      hipStream_t cst = st;
      if (side != nullptr) {
        TRANSOAR_CHECK_HIP(hipEventRecord(side->fork, st));
        TRANSOAR_CHECK_HIP(hipStreamWaitEvent(side->stream, side->fork, 0));
        cst = side->stream;
      }
      if (coarse_levels > 0) {
        ProfScope prof(TRANSOAR_PROF_VALUE_CELLS, cst);
        TRANSOAR_CHECK_HIP(zero_async(scratch, sizeof(float) * scratch_elems, cst));
        const long waves = static_cast<long>(d.N) * d.M * cl.chunks_per_slab;
        if (mma) {
          if constexpr (sizeof(VT) == 2)       // 16 sorted points per MFMA K-step (msda3d_cells_mma.hpp)
            hipLaunchKernelGGL((msda3d_bwd_value_cells_mma<VT>), dim3(static_cast<unsigned>((waves + 3) / 4)), dim3(256), 0,
                               cst, go, offsets, recs4, scratch, cells, d.N * d.M, d.M, cl_d, r_order_d);
        } else {
          hipLaunchKernelGGL((msda3d_bwd_value_cells<VT>), dim3(static_cast<unsigned>((waves + 3) / 4)), dim3(256), 0, cst,
                             go, count, recs8, rec_item, scratch, cells, d.N * d.M, d.M, cl_d, r_order_d);
        }
      }
      if (side != nullptr) TRANSOAR_CHECK_HIP(hipEventRecord(side->join, side->stream));
      ProfScope prof(TRANSOAR_PROF_VALUE_TILE, st);
      if (fine_bricks > 0) {
        const long n_wg = static_cast<long>(d.N) * fine_bricks * d.M;
        if (mma) {
          if constexpr (sizeof(VT) == 2)
            hipLaunchKernelGGL((msda3d_bwd_value_tile_mma<VT>), dim3(static_cast<unsigned>(n_wg)), dim3(kBrickThreads), 0, st,
                               go, offsets, recs4, gv, cells, d.S, d.M, fine_bricks, n_wg, r_order_d);
        } else {
          hipLaunchKernelGGL((msda3d_bwd_value_tile<VT>), dim3(static_cast<unsigned>(n_wg)), dim3(kBrickThreads), 0, st, go,
                             count, recs8, rec_item, gv, cells, d.S, d.M, fine_bricks, n_wg, r_order_d);
        }
      }
      if (side != nullptr) TRANSOAR_CHECK_HIP(hipStreamWaitEvent(st, side->join, 0));
      if (coarse_levels > 0) {
        const long n4 = scratch_elems / 4;
        hipLaunchKernelGGL((msda3d_coarse_rows_store<VT>), dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, st,
                           scratch, gv, d.S, d.M, cl.rows, cl.row_start, n4);
      }
    }
    return static_cast<int>(hipGetLastError());
  }

  // voxel-stationary pull over PointRec records
  int value_pull() const {
    auto recs = reinterpret_cast<PointRec<A>*>(ws + p.ws.recs);
    {
      ProfScope prof(TRANSOAR_PROF_CELL_FILL, st);
      hipLaunchKernelGGL((msda3d_cell_fill<LT, A>), pgrid, dim3(256), 0, st, lo, at, shapes, lsi, count,
                         rank, recs, rec_item, d.M, d.L, d.Lq, d.P, p.ws.n_points);
    }
    const long n_rows = order_units(p.r_order, d, d.S);
    const long r_blocks = (n_rows + kWavesPerBlock - 1) / kWavesPerBlock;
    const dim3 rgrid(((r_blocks + 7) / 8) * 8);
#define TRANSOAR_PULL(LG)                                                                        \
  hipLaunchKernelGGL((msda3d_bwd_value_pull<VT, A, LG>), rgrid, block, 0, st, go, shapes, lsi, count, \
                     recs, rec_item, gv, d.S, d.M, d.C, d.L, n_rows, r_blocks, p.r_order, \
                     static_cast<unsigned>(p.ws.n_points * 4 * sizeof(A)))
    ProfScope prof(TRANSOAR_PROF_PULL, st);
    TRANSOAR_BY_LG(p.lg, TRANSOAR_PULL);
#undef TRANSOAR_PULL
    return static_cast<int>(hipGetLastError());
  }
};

template <typename VT, typename LT>
static int launch_bwd(const void* value, const int64_t* shapes, const int64_t* lsi, const void* loc, const void* attn,
                      const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn, void* grad_proj,
                      void* workspace, size_t workspace_bytes, const Dims& d, const int64_t* host_shapes, unsigned flags,
                      hipStream_t st) {
  // grad_proj: the sampling head's backward folded into the query kernel (transoar_msda3d_backward_proj)
  const BwdPlan p = plan_bwd(d, sizeof(VT), sizeof(LT), host_shapes, flags, grad_proj != nullptr);
  if (workspace_bytes < p.ws.total) return TRANSOAR_ERR_WORKSPACE;
  if (p.status != TRANSOAR_OK) return p.status;          // refused before anything is launched
  const BwdLaunch<VT, LT> c{d, p, st, static_cast<char*>(workspace), shapes, lsi, static_cast<const VT*>(value),
                            static_cast<const VT*>(grad_out), static_cast<const LT*>(loc), static_cast<const LT*>(attn),
                            static_cast<VT*>(grad_value), static_cast<LT*>(grad_loc), static_cast<LT*>(grad_attn),
                            static_cast<unsigned short*>(grad_proj), (flags & TRANSOAR_MSDA3D_FORK) != 0};
  return c.run();
}

static int check_common(const Dims& d, int value_dtype, int loc_dtype) {
  if (d.N <= 0 || d.S <= 0 || d.M <= 0 || d.C <= 0 || d.L <= 0 || d.Lq <= 0 || d.P <= 0)
    return TRANSOAR_ERR_DIM;
  if (d.L > TRANSOAR_MSDA3D_MAX_LEVELS) return TRANSOAR_ERR_LEVELS;
  // item index and row index are 32-bit inside the kernels
  if (static_cast<long>(d.N) * d.Lq * d.M >= (1L << 31) || static_cast<long>(d.N) * d.S >= (1L << 31))
    return TRANSOAR_ERR_DIM;
  const bool half = value_dtype == TRANSOAR_BF16 || value_dtype == TRANSOAR_F16;
  if (value_dtype < 0 || value_dtype > TRANSOAR_F16) return TRANSOAR_ERR_DTYPE;
  if (!(loc_dtype == value_dtype || (half && loc_dtype == TRANSOAR_F32))) return TRANSOAR_ERR_DTYPE;
  return TRANSOAR_OK;
}

static inline int elt_size(int dtype) { return dtype == TRANSOAR_F32 ? 4 : dtype == TRANSOAR_F64 ? 8 : 2; }
static inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace transoar

using namespace transoar;

#define TRANSOAR_DISPATCH(VD, LD, CALL)                                            \
  do {                                                                             \
    if (VD == TRANSOAR_F32) { using VT = float; using LT = float; return CALL; }   \
    if (VD == TRANSOAR_F64) { using VT = double; using LT = double; return CALL; } \
    if (VD == TRANSOAR_BF16 && LD == TRANSOAR_BF16) { using VT = bf16_t; using LT = bf16_t; return CALL; } \
    if (VD == TRANSOAR_BF16) { using VT = bf16_t; using LT = float; return CALL; } \
    if (VD == TRANSOAR_F16 && LD == TRANSOAR_F16) { using VT = f16_t; using LT = f16_t; return CALL; }     \
    { using VT = f16_t; using LT = float; return CALL; }                           \
  } while (0)

extern "C" int transoar_msda3d_forward(const void* value, const int64_t* spatial_shapes,
                                       const int64_t* level_start_index, const void* sampling_loc,
                                       const void* attn_weight, void* out, int N, int S, int M,
                                       int C, int L, int Lq, int P, int value_dtype, int loc_dtype,
                                       const int64_t* host_spatial_shapes, unsigned flags,
                                       void* hip_stream) {
  if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight || !out)
    return TRANSOAR_ERR_NULL;
  const Dims d{N, S, M, C, L, Lq, P};
  const int rc = check_common(d, value_dtype, loc_dtype);
  if (rc != TRANSOAR_OK) return rc;
  if (misaligned(value) || misaligned(sampling_loc) || misaligned(attn_weight) || misaligned(out))
    return TRANSOAR_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  TRANSOAR_DISPATCH(value_dtype, loc_dtype,
                    (launch_fwd<VT, LT>(value, spatial_shapes, level_start_index, sampling_loc,
                                        attn_weight, out, d, host_spatial_shapes, flags, st)));
}

extern "C" int transoar_msda3d_forward_fused(const void* value, const void* proj, const float* ref, long ref_rows,
                                             void* out, int N, int S, int M, int C, int L, int P, int value_dtype,
                                             const int64_t* host_spatial_shapes, void* hip_stream) {
  if (!value || !proj || !ref || !out || !host_spatial_shapes) return TRANSOAR_ERR_NULL;
  const Dims d{N, S, M, C, L, S, P};
  const int rc = check_common(d, value_dtype, TRANSOAR_F32);
  if (rc != TRANSOAR_OK) return rc;
  if (value_dtype != TRANSOAR_BF16 && value_dtype != TRANSOAR_F16) return TRANSOAR_ERR_DTYPE;
  if (misaligned(value) || misaligned(proj) || misaligned(ref) || misaligned(out)) return TRANSOAR_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (value_dtype == TRANSOAR_BF16) return launch_fwd_fused<bf16_t>(value, proj, ref, ref_rows, out, d, host_spatial_shapes, st);
  return launch_fwd_fused<f16_t>(value, proj, ref, ref_rows, out, d, host_spatial_shapes, st);
}

// what the two backward entry points share; grad_proj != NULL: transoar_msda3d_backward_proj (no grad_loc / grad_attn)
static int backward_entry(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                          const void* sampling_loc, const void* attn_weight, const void* grad_out, void* grad_value,
                          void* grad_loc, void* grad_attn, void* grad_proj, void* workspace, size_t workspace_bytes,
                          const Dims& d, int value_dtype, int loc_dtype, const int64_t* host_shapes, unsigned flags,
                          void* hip_stream) {
  if (!value || !spatial_shapes || !level_start_index || !sampling_loc || !attn_weight || !grad_out || !grad_value ||
      (!grad_proj && (!grad_loc || !grad_attn)))
    return TRANSOAR_ERR_NULL;
  const int rc = check_common(d, value_dtype, loc_dtype);
  if (rc != TRANSOAR_OK) return rc;
  if (grad_proj && !proj_form(d, elt_size(value_dtype), elt_size(loc_dtype))) return TRANSOAR_ERR_MODE;
  if (misaligned(value) || misaligned(sampling_loc) || misaligned(attn_weight) || misaligned(grad_out) ||
      misaligned(grad_value) || misaligned(grad_loc) || misaligned(grad_attn) || misaligned(grad_proj) || misaligned(workspace))
    return TRANSOAR_ERR_ALIGN;
  if (!workspace && workspace_bytes != 0) return TRANSOAR_ERR_NULL;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  TRANSOAR_DISPATCH(value_dtype, loc_dtype,
                    (launch_bwd<VT, LT>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out,
                                        grad_value, grad_loc, grad_attn, grad_proj, workspace, workspace_bytes, d,
                                        host_shapes, flags, st)));
}

extern "C" int transoar_msda3d_backward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                        const void* sampling_loc, const void* attn_weight, const void* grad_out,
                                        void* grad_value, void* grad_sampling_loc, void* grad_attn_weight, void* workspace,
                                        size_t workspace_bytes, int N, int S, int M, int C, int L, int Lq, int P,
                                        int value_dtype, int loc_dtype, const int64_t* host_spatial_shapes, unsigned flags,
                                        void* hip_stream) {
  return backward_entry(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, grad_value,
                        grad_sampling_loc, grad_attn_weight, nullptr, workspace, workspace_bytes, Dims{N, S, M, C, L, Lq, P},
                        value_dtype, loc_dtype, host_spatial_shapes, flags, hip_stream);
}

extern "C" int transoar_msda3d_backward_proj(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                             const void* sampling_loc, const void* attn_weight, const void* grad_out,
                                             void* grad_value, void* grad_proj, void* workspace, size_t workspace_bytes,
                                             int N, int S, int M, int C, int L, int Lq, int P, int value_dtype, int loc_dtype,
                                             const int64_t* host_spatial_shapes, unsigned flags, void* hip_stream) {
  return backward_entry(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, grad_value,
                        nullptr, nullptr, grad_proj, workspace, workspace_bytes, Dims{N, S, M, C, L, Lq, P},
                        value_dtype, loc_dtype, host_spatial_shapes, flags, hip_stream);
}

extern "C" size_t transoar_msda3d_backward_workspace_bytes(int N, int S, int M, int C, int L, int Lq,
                                                           int P, int value_dtype, int loc_dtype,
                                                           unsigned flags) {
  const Dims d{N, S, M, C, L, Lq, P};
  if (check_common(d, value_dtype, loc_dtype) != TRANSOAR_OK) return 0;
  return plan_bwd(d, elt_size(value_dtype), elt_size(loc_dtype), nullptr, flags, false).ws.total;
}

extern "C" int transoar_msda3d_plan(int N, int S, int M, int C, int L, int Lq, int P, int value_dtype, int loc_dtype,
                                    const int64_t* host_spatial_shapes, unsigned flags, int grad_proj, int* plan) {
  if (!plan) return TRANSOAR_ERR_NULL;
  const Dims d{N, S, M, C, L, Lq, P};
  const int rc = check_common(d, value_dtype, loc_dtype);
  if (rc != TRANSOAR_OK) return rc;
  const int vs = elt_size(value_dtype), ls = elt_size(loc_dtype);
  const BwdPlan b = plan_bwd(d, vs, ls, host_spatial_shapes, flags, grad_proj != 0);
  const bool ok = b.status == TRANSOAR_OK;
  plan[TRANSOAR_PLAN_FWD] = plan_fwd(d, vs, ls, host_spatial_shapes, flags).kernel;
  plan[TRANSOAR_PLAN_BWD_QUERY] = ok ? b.query : -1;
  plan[TRANSOAR_PLAN_BWD_VALUE] = ok ? b.value : -1;
  plan[TRANSOAR_PLAN_COARSE_FIRST] = ok ? b.coarse.first : -1;
  return b.status;
}

extern "C" const char* transoar_msda3d_strerror(int code) {
  switch (code) {
    case TRANSOAR_OK: return "success";
    case TRANSOAR_ERR_NULL: return "a required pointer is NULL";
    case TRANSOAR_ERR_DIM: return "a dimension is non-positive or exceeds the 32-bit index range";
    case TRANSOAR_ERR_DTYPE: return "unsupported value/loc dtype combination";
    case TRANSOAR_ERR_ALIGN: return "a device buffer is not 16-byte aligned";
    case TRANSOAR_ERR_LEVELS: return "too many feature levels";
    case TRANSOAR_ERR_WORKSPACE: return "workspace is smaller than transoar_msda3d_backward_workspace_bytes()";
    case TRANSOAR_ERR_MODE: return "the deterministic backward does not cover this form (16-bit storage, C = 64, P = 4, <= 4 host-known levels, queries = pyramid voxels)";
    case TRANSOAR_ERR_CONST: return "could not place the launch constants in device memory (first call for a shape must not be inside a stream capture)";
    default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "unknown error";
  }
}

extern "C" void transoar_msda3d_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
}

extern "C" int transoar_msda3d_profile_read(double* total_ms, long* launches) {
  std::vector<ProfPair> live;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    live.swap(g_prof_live);
  }
  for (int k = 0; k < TRANSOAR_PROF_KINDS; ++k) {
    total_ms[k] = 0.0;
    launches[k] = 0;
  }
  int rc = 0;
  for (const ProfPair& p : live) {
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(p.end);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.beg, p.end);
    if (e != hipSuccess) { rc = static_cast<int>(e); continue; }
    total_ms[p.kind] += ms;
    launches[p.kind] += 1;
  }
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_free.insert(g_prof_free.end(), live.begin(), live.end());
  return rc;
}

extern "C" int transoar_msda3d_abi_version(void) { return 7; }
