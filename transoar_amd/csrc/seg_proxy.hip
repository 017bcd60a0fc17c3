// Segmentation proxy loss for gfx950 (include/transoar_segproxy.h): the 1x1x1 segmentation head on the full-resolution FPN
// level P0 and the softmax cross-entropy + batch soft-Dice losses of transoar/models/criterion.py:77-90,127-197.
//
// Everything here is a streaming pass over N * S voxels (13.1 M at the flagship's batch 2) with a handful of flops per byte.
//   * head forward / backward: a workgroup stages a tile of kTile voxels (features, and the logit gradient in the backward) in LDS
//     as fp32, so that both layouts are read and written as contiguous runs whatever the channel count; the tile's outputs are
//     computed from LDS.  The weight / bias gradients are per-thread register sums over the tiles a workgroup visits (a thread
//     owns fixed (k, c) pairs), written as one fp32 slab per workgroup and summed in a fixed order by a second launch.
//   * loss forward: a thread owns a voxel at a time (the K logits of a voxel in registers): log-softmax, the CE term and the
//     per-class sums tp_k, P_k, Y_k in fp32 registers; wave then workgroup reductions in a fixed order into a per-workgroup slab;
//     a one-workgroup launch sums the slabs (fp64, fixed order) and finalises segce, segdice and the Dice numerators /
//     denominators the backward needs.
//   * loss backward: the same per-voxel pass, recomputing the softmax, with the Dice gradient's per-class coefficients formed once
//     per workgroup from the saved statistics and the upstream gradients read on the device.
// The number of workgroups depends only on the shape, so every result is bitwise reproducible (no float atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/transoar_segproxy.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;                 // voxels per LDS tile of the head kernels
constexpr int kHeadFwdBlocks = 8192;      // cap of the head forward's grid (grid-stride over the tiles)
constexpr int kHeadBwdBlocks = 1024;      // workgroups (= partial slabs) of the head backward: 4 per CU at 33 KB of LDS each
constexpr int kLossBlocks = 1024;         // workgroups (= partial slabs) of the loss forward
constexpr int kMaxAcc = 1 + 3 * TRANSOAR_SEG_MAX_K;
constexpr int kMaxPairs = TRANSOAR_SEG_MAX_K * TRANSOAR_SEG_MAX_C + TRANSOAR_SEG_MAX_K;

template <typename T> __device__ __forceinline__ float load_f(const void* p, long i);
template <> __device__ __forceinline__ float load_f<float>(const void* p, long i) { return static_cast<const float*>(p)[i]; }
template <> __device__ __forceinline__ float load_f<unsigned short>(const void* p, long i) {
  return __uint_as_float(static_cast<unsigned>(static_cast<const unsigned short*>(p)[i]) << 16);
}
__device__ __forceinline__ unsigned short bf16_rne(float x) {
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<unsigned short>((u >> 16) | 0x40u);      // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<unsigned short>(u >> 16);
}
template <typename T> __device__ __forceinline__ void store_f(void* p, long i, float v);
template <> __device__ __forceinline__ void store_f<float>(void* p, long i, float v) { static_cast<float*>(p)[i] = v; }
template <> __device__ __forceinline__ void store_f<unsigned short>(void* p, long i, float v) {
  static_cast<unsigned short*>(p)[i] = bf16_rne(v);
}

// label of voxel i as a class index in [0, K): (label > 0) under fg_bg; out-of-range values (a caller error) are clamped so that
// they cannot index outside a buffer
__device__ __forceinline__ int load_label(const void* p, int dt, long i, int fg_bg, int K) {
  long l;
  switch (dt) {
    case TRANSOAR_SEG_U8: l = static_cast<const unsigned char*>(p)[i]; break;
    case TRANSOAR_SEG_I16: l = static_cast<const short*>(p)[i]; break;
    case TRANSOAR_SEG_I32: l = static_cast<const int*>(p)[i]; break;
    default: l = static_cast<const long long*>(p)[i]; break;
  }
  if (fg_bg) l = l > 0 ? 1 : 0;
  return static_cast<int>(l < 0 ? 0 : (l >= K ? K - 1 : l));
}

// element offset of (voxel v, channel c) of a map with CH channels; v = n * S + s
__device__ __forceinline__ long map_base(int layout, long v, long S, int CH) {
  if (layout == TRANSOAR_SEG_NDHWC) return v * CH;
  const long n = v / S;
  return n * CH * S + (v - n * S);
}

// tile of nv voxels from v0 on -> dst[vl * pitch + c] (fp32); contiguous global runs in both layouts
template <typename T>
__device__ __forceinline__ void load_tile(const void* src, int layout, long v0, int nv, int CH, long S, float* dst, int pitch) {
  if (layout == TRANSOAR_SEG_NDHWC) {
    const long base = v0 * CH;
    for (int i = threadIdx.x; i < nv * CH; i += kThreads) {
      const int vl = i / CH;
      dst[vl * pitch + (i - vl * CH)] = load_f<T>(src, base + i);
    }
  } else {
    for (int i = threadIdx.x; i < nv * CH; i += kThreads) {
      const int c = i / nv, vl = i - c * nv;
      dst[vl * pitch + c] = load_f<T>(src, map_base(layout, v0 + vl, S, CH) + static_cast<long>(c) * S);
    }
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- head ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void seg_head_fwd(const void* x, int xl, const float* w, const float* b, long V, long S, int C,
                                                          int K, void* y) {
  __shared__ float xs[kTile * (TRANSOAR_SEG_MAX_C + 1)];
  __shared__ float ws[TRANSOAR_SEG_MAX_K * (TRANSOAR_SEG_MAX_C + 1)];
  __shared__ float bs[TRANSOAR_SEG_MAX_K];
  const int CP = C | 1;                   // odd row pitches: no bank conflicts between rows
  for (int i = threadIdx.x; i < K * C; i += kThreads) ws[(i / C) * CP + i % C] = w[i];
  if (threadIdx.x < K) bs[threadIdx.x] = b[threadIdx.x];
  const long tiles = (V + kTile - 1) / kTile;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long v0 = t * kTile;
    const int nv = static_cast<int>(V - v0 < kTile ? V - v0 : kTile);
    __syncthreads();                      // the previous tile's readers are done (first pass: ws / bs are visible)
    load_tile<T>(x, xl, v0, nv, C, S, xs, CP);
    __syncthreads();
    for (int i = threadIdx.x; i < nv * K; i += kThreads) {       // y is channels-last: the tile's outputs are one run
      const int vl = i / K, k = i - vl * K;
      const float* xr = xs + vl * CP;
      const float* wr = ws + k * CP;
      float acc = bs[k];
      for (int c = 0; c < C; ++c) acc = fmaf(wr[c], xr[c], acc);
      store_f<T>(y, v0 * K + i, acc);
    }
  }
}

// NP = (k, c) pairs per thread: pair p < K*C is dw[p / C, p % C], K*C <= p < K*C + K is db[p - K*C]
template <typename T, int NP>
__global__ __launch_bounds__(kThreads) void seg_head_bwd(const void* x, int xl, const void* dy, int dyl, const float* w, long V, long S,
                                                          int C, int K, void* dx, float* part) {
  __shared__ float xs[kTile * (TRANSOAR_SEG_MAX_C + 1)];
  __shared__ float dys[kTile * (TRANSOAR_SEG_MAX_K + 1)];
  __shared__ float ws[TRANSOAR_SEG_MAX_K * (TRANSOAR_SEG_MAX_C + 1)];
  const int CP = C | 1, KP = K | 1, KC = K * C, P = KC + K;
  for (int i = threadIdx.x; i < KC; i += kThreads) ws[(i / C) * CP + i % C] = w[i];
  int pk[NP], pc[NP];
  float acc[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = threadIdx.x + j * kThreads;
    pk[j] = p < KC ? p / C : (p < P ? p - KC : -1);
    pc[j] = p < KC ? p % C : -1;
    acc[j] = 0.f;
  }
  const long tiles = (V + kTile - 1) / kTile;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long v0 = t * kTile;
    const int nv = static_cast<int>(V - v0 < kTile ? V - v0 : kTile);
    __syncthreads();
    load_tile<T>(x, xl, v0, nv, C, S, xs, CP);
    load_tile<T>(dy, dyl, v0, nv, K, S, dys, KP);
    __syncthreads();
    if (dx) {
      for (int i = threadIdx.x; i < nv * C; i += kThreads) {
        int vl, c;
        long o;
        if (xl == TRANSOAR_SEG_NDHWC) {
          vl = i / C;
          c = i - vl * C;
          o = v0 * C + i;
        } else {
          c = i / nv;
          vl = i - c * nv;
          o = map_base(xl, v0 + vl, S, C) + static_cast<long>(c) * S;
        }
        const float* dr = dys + vl * KP;
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = fmaf(ws[k * CP + c], dr[k], a);
        store_f<T>(dx, o, a);
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (pk[j] < 0) continue;
      const float* dr = dys + pk[j];
      float a = acc[j];
      if (pc[j] >= 0) {
        const float* xr = xs + pc[j];
        for (int vl = 0; vl < nv; ++vl) a = fmaf(dr[vl * KP], xr[vl * CP], a);
      } else {
        for (int vl = 0; vl < nv; ++vl) a += dr[vl * KP];
      }
      acc[j] = a;
    }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = threadIdx.x + j * kThreads;
    if (p < P) part[static_cast<long>(blockIdx.x) * P + p] = acc[j];
  }
}

// one wave per output: lanes stride over the slabs, fp64, then a fixed-order wave sum
__global__ __launch_bounds__(1024) void seg_head_bwd_reduce(const float* part, int nb, int K, int C, float* dw, float* db) {
  const int P = K * C + K;
  const int p = blockIdx.x * 16 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;                     // whole waves leave together
  double s = 0.0;
  for (int b = lane; b < nb; b += 64) s += part[static_cast<long>(b) * P + p];
  s = wave_sum_d(s);
  if (lane == 0) {
    if (p < K * C) dw[p] = static_cast<float>(s);
    else db[p - K * C] = static_cast<float>(s);
  }
}

// ---- losses ----------------------------------------------------------------------------------------------------------------
template <typename T, int KM>
__global__ __launch_bounds__(kThreads) void seg_loss_fwd(const void* logits, int layout, const void* labels, int ldt, long V, long S,
                                                          int K, int fg_bg, float* part) {
  __shared__ float red[kThreads / 64][kMaxAcc];
  float ce = 0.f, tp[KM], pp[KM], yy[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) tp[k] = pp[k] = yy[k] = 0.f;
  const long step = static_cast<long>(gridDim.x) * kThreads;
  for (long v = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; v < V; v += step) {
    const long base = map_base(layout, v, S, K);
    const long cs = layout == TRANSOAR_SEG_NDHWC ? 1 : S;
    const int y = load_label(labels, ldt, v, fg_bg, K);
    float z[KM];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        z[k] = load_f<T>(logits, base + k * cs);
        m = fmaxf(m, z[k]);
      }
    }
    float se = 0.f, zy = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        zy = k == y ? z[k] : zy;
        z[k] = expf(z[k] - m);
        se += z[k];
      }
    }
    ce += logf(se) + m - zy;
    const float inv = 1.f / se;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        const float p = z[k] * inv;
        pp[k] += p;
        tp[k] += k == y ? p : 0.f;
        yy[k] += k == y ? 1.f : 0.f;
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  ce = wave_sum(ce);
  if (lane == 0) red[wave][0] = ce;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (k < K) {
      const float a = wave_sum(tp[k]), b = wave_sum(pp[k]), c = wave_sum(yy[k]);
      if (lane == 0) {
        red[wave][1 + k] = a;
        red[wave][1 + K + k] = b;
        red[wave][1 + 2 * K + k] = c;
      }
    }
  }
  __syncthreads();
  const int A = 1 + 3 * K;
  if (threadIdx.x < A) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < kThreads / 64; ++wv) s += red[wv][threadIdx.x];
    part[static_cast<long>(blockIdx.x) * A + threadIdx.x] = s;
  }
}

// one workgroup of 16 waves: wave w sums accumulators w, w + 16, ... over the slabs (lanes stride over them, fp64, fixed-order wave
// sum), then segce, the Dice terms and segdice
__global__ __launch_bounds__(1024) void seg_loss_finalize(const float* part, int nb, long V, int K, float sn, float sd, float* losses,
                                                           float* stats) {
  __shared__ double tot[kMaxAcc];
  __shared__ double dc[TRANSOAR_SEG_MAX_K];
  const int A = 1 + 3 * K;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < A; i += 16) {
    double s = 0.0;
    for (int b = lane; b < nb; b += 64) s += part[static_cast<long>(b) * A + i];
    s = wave_sum_d(s);
    if (lane == 0) tot[i] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    const double num = 2.0 * tot[1 + k] + sn, den = tot[1 + K + k] + tot[1 + 2 * K + k] + sd;
    dc[k] = num / den;
    stats[k] = static_cast<float>(num);
    stats[K + k] = static_cast<float>(den);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 1; k < K; ++k) s += dc[k];
    losses[0] = static_cast<float>(tot[0] / static_cast<double>(V));
    losses[1] = static_cast<float>(1.0 - s / (K - 1));
  }
}

template <typename T, int KM>
__global__ __launch_bounds__(kThreads) void seg_loss_bwd(const void* logits, int layout, const void* labels, int ldt, long V, long S,
                                                          int K, int fg_bg, const float* stats, const float* g, void* grad) {
  __shared__ float c0[KM], c1[KM];
  if (threadIdx.x < K) {
    // a_k = dL/dp_k of the Dice term = c0_k + [y = k] c1_k  (k >= 1; the background class is not in the mean)
    const int k = threadIdx.x;
    const float gd = g[1] / static_cast<float>(K - 1);
    const float num = stats[k], den = stats[K + k];
    c0[k] = k == 0 ? 0.f : gd * num / (den * den);
    c1[k] = k == 0 ? 0.f : -2.f * gd / den;
  }
  __syncthreads();
  const float gce = g[0] / static_cast<float>(V);
  const long step = static_cast<long>(gridDim.x) * kThreads;
  for (long v = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; v < V; v += step) {
    const long base = map_base(layout, v, S, K);
    const long cs = layout == TRANSOAR_SEG_NDHWC ? 1 : S;
    const int y = load_label(labels, ldt, v, fg_bg, K);
    float z[KM];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        z[k] = load_f<T>(logits, base + k * cs);
        m = fmaxf(m, z[k]);
      }
    }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        z[k] = expf(z[k] - m);
        se += z[k];
      }
    }
    const float inv = 1.f / se;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        z[k] *= inv;                                          // p_k
        s = fmaf(z[k], c0[k] + (k == y ? c1[k] : 0.f), s);    // sum_j p_j a_j
      }
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < K) {
        const float a = c0[k] + (k == y ? c1[k] : 0.f);
        const float d = z[k] * (a - s) + gce * (z[k] - (k == y ? 1.f : 0.f));
        store_f<T>(grad, base + k * cs, d);
      }
    }
  }
}

bool dtype_ok(int dt) { return dt == TRANSOAR_SEG_F32 || dt == TRANSOAR_SEG_BF16; }
bool layout_ok(int l) { return l == TRANSOAR_SEG_NCDHW || l == TRANSOAR_SEG_NDHWC; }
bool label_ok(int dt) { return dt == TRANSOAR_SEG_U8 || dt == TRANSOAR_SEG_I16 || dt == TRANSOAR_SEG_I32 || dt == TRANSOAR_SEG_I64; }
bool shape_ok(long N, long S) { return N >= 1 && S >= 1 && N <= (1L << 40) / S; }
long tiles_of(long V) { return (V + kTile - 1) / kTile; }
int loss_blocks(long V) {
  const long b = (V + kThreads - 1) / kThreads;
  return static_cast<int>(b < kLossBlocks ? b : kLossBlocks);
}

}  // namespace

extern "C" size_t transoar_seg_workspace_bytes(int C, int K) {
  if (C < 0 || C > TRANSOAR_SEG_MAX_C || K < 1 || K > TRANSOAR_SEG_MAX_K) return 0;
  const size_t head = static_cast<size_t>(kHeadBwdBlocks) * (K * C + K);
  const size_t loss = static_cast<size_t>(kLossBlocks) * (1 + 3 * K);
  return 4 * (head > loss ? head : loss);
}

extern "C" int transoar_seg_head_forward(const void* x, int x_layout, int dtype, const float* weight, const float* bias, long N, long S,
                                         int C, int K, void* y, void* hip_stream) {
  if (!x || !weight || !bias || !y) return TRANSOAR_SEG_ERR_NULL;
  if (!shape_ok(N, S) || C < 1 || C > TRANSOAR_SEG_MAX_C || K < 1 || K > TRANSOAR_SEG_MAX_K) return TRANSOAR_SEG_ERR_DIM;
  if (!dtype_ok(dtype)) return TRANSOAR_SEG_ERR_DTYPE;
  if (!layout_ok(x_layout)) return TRANSOAR_SEG_ERR_LAYOUT;
  const long V = N * S, tiles = tiles_of(V);
  const dim3 grid(static_cast<unsigned>(tiles < kHeadFwdBlocks ? tiles : kHeadFwdBlocks));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (dtype == TRANSOAR_SEG_F32)
    hipLaunchKernelGGL(seg_head_fwd<float>, grid, dim3(kThreads), 0, st, x, x_layout, weight, bias, V, S, C, K, y);
  else
    hipLaunchKernelGGL(seg_head_fwd<unsigned short>, grid, dim3(kThreads), 0, st, x, x_layout, weight, bias, V, S, C, K, y);
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_seg_head_backward(const void* x, int x_layout, int dtype, const void* dy, int dy_layout, const float* weight,
                                          long N, long S, int C, int K, void* dx, float* dw, float* db, float* workspace,
                                          void* hip_stream) {
  if (!x || !dy || !weight || !dw || !db || !workspace) return TRANSOAR_SEG_ERR_NULL;
  if (!shape_ok(N, S) || C < 1 || C > TRANSOAR_SEG_MAX_C || K < 1 || K > TRANSOAR_SEG_MAX_K) return TRANSOAR_SEG_ERR_DIM;
  if (!dtype_ok(dtype)) return TRANSOAR_SEG_ERR_DTYPE;
  if (!layout_ok(x_layout) || !layout_ok(dy_layout)) return TRANSOAR_SEG_ERR_LAYOUT;
  const long V = N * S, tiles = tiles_of(V);
  const int nb = static_cast<int>(tiles < kHeadBwdBlocks ? tiles : kHeadBwdBlocks);
  const int P = K * C + K, np = (P + kThreads - 1) / kThreads;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
#define TRANSOAR_SEG_LAUNCH(T, NP) \
  hipLaunchKernelGGL((seg_head_bwd<T, NP>), dim3(nb), dim3(kThreads), 0, st, x, x_layout, dy, dy_layout, weight, V, S, C, K, dx, workspace)
#define TRANSOAR_SEG_BY_NP(T)                 \
  if (np <= 1) TRANSOAR_SEG_LAUNCH(T, 1);     \
  else if (np <= 2) TRANSOAR_SEG_LAUNCH(T, 2); \
  else if (np <= 4) TRANSOAR_SEG_LAUNCH(T, 4); \
  else TRANSOAR_SEG_LAUNCH(T, 9)
  static_assert(kMaxPairs <= 9 * kThreads, "pairs per thread");
  if (dtype == TRANSOAR_SEG_F32) {
    TRANSOAR_SEG_BY_NP(float);
  } else {
    TRANSOAR_SEG_BY_NP(unsigned short);
  }
#undef TRANSOAR_SEG_BY_NP
#undef TRANSOAR_SEG_LAUNCH
  hipLaunchKernelGGL(seg_head_bwd_reduce, dim3((P + 15) / 16), dim3(1024), 0, st, workspace, nb, K, C, dw, db);
  return static_cast<int>(hipGetLastError());
}

#define TRANSOAR_SEG_BY_K(LAUNCH, T) \
  if (K <= 2) LAUNCH(T, 2);          \
  else if (K <= 4) LAUNCH(T, 4);     \
  else if (K <= 8) LAUNCH(T, 8);     \
  else if (K <= 16) LAUNCH(T, 16);   \
  else LAUNCH(T, 32)

extern "C" int transoar_seg_loss_forward(const void* logits, int layout, int dtype, const void* labels, int label_dtype, long N, long S,
                                         int K, int fg_bg, float smooth_nom, float smooth_denom, float* losses, float* stats,
                                         float* workspace, void* hip_stream) {
  if (!logits || !labels || !losses || !stats || !workspace) return TRANSOAR_SEG_ERR_NULL;
  if (!shape_ok(N, S) || K < 2 || K > TRANSOAR_SEG_MAX_K) return TRANSOAR_SEG_ERR_DIM;
  if (!dtype_ok(dtype) || !label_ok(label_dtype)) return TRANSOAR_SEG_ERR_DTYPE;
  if (!layout_ok(layout)) return TRANSOAR_SEG_ERR_LAYOUT;
  const long V = N * S;
  const int nb = loss_blocks(V);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
#define TRANSOAR_SEG_LAUNCH(T, KM) \
  hipLaunchKernelGGL((seg_loss_fwd<T, KM>), dim3(nb), dim3(kThreads), 0, st, logits, layout, labels, label_dtype, V, S, K, fg_bg != 0, workspace)
  if (dtype == TRANSOAR_SEG_F32) {
    TRANSOAR_SEG_BY_K(TRANSOAR_SEG_LAUNCH, float);
  } else {
    TRANSOAR_SEG_BY_K(TRANSOAR_SEG_LAUNCH, unsigned short);
  }
#undef TRANSOAR_SEG_LAUNCH
  hipLaunchKernelGGL(seg_loss_finalize, dim3(1), dim3(1024), 0, st, workspace, nb, V, K, smooth_nom, smooth_denom, losses, stats);
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_seg_loss_backward(const void* logits, int layout, int dtype, const void* labels, int label_dtype, long N, long S,
                                          int K, int fg_bg, const float* stats, const float* g, void* grad_logits, void* hip_stream) {
  if (!logits || !labels || !stats || !g || !grad_logits) return TRANSOAR_SEG_ERR_NULL;
  if (!shape_ok(N, S) || K < 2 || K > TRANSOAR_SEG_MAX_K) return TRANSOAR_SEG_ERR_DIM;
  if (!dtype_ok(dtype) || !label_ok(label_dtype)) return TRANSOAR_SEG_ERR_DTYPE;
  if (!layout_ok(layout)) return TRANSOAR_SEG_ERR_LAYOUT;
  const long V = N * S;
  const int nb = loss_blocks(V);          // no reduction here: any grid would do, the forward's is a good one
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
#define TRANSOAR_SEG_LAUNCH(T, KM)                                                                                            \
  hipLaunchKernelGGL((seg_loss_bwd<T, KM>), dim3(nb), dim3(kThreads), 0, st, logits, layout, labels, label_dtype, V, S, K, fg_bg != 0, \
                     stats, g, grad_logits)
  if (dtype == TRANSOAR_SEG_F32) {
    TRANSOAR_SEG_BY_K(TRANSOAR_SEG_LAUNCH, float);
  } else {
    TRANSOAR_SEG_BY_K(TRANSOAR_SEG_LAUNCH, unsigned short);
  }
#undef TRANSOAR_SEG_LAUNCH
  return static_cast<int>(hipGetLastError());
}

#undef TRANSOAR_SEG_BY_K

extern "C" int transoar_segproxy_abi_version(void) { return 1; }
