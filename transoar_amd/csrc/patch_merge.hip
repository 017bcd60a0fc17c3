// Convolutional patch merging of the Swin encoder (Conv3d(C, 2C, kernel 2, stride 2), no bias) on a channels-last token
// map, gfx950: C ABI include/transoar_patchmerge.h, design DESIGN.md section 12.15.
//
// With the weights packed to (2C, [kd, kh, kw, c]) the convolution is one GEMM  Y (M x 2C) = A (M x 8C) . Wp^T  whose
// A rows are never formed: row m = (b, d', h', w') is four K segments of 2C contiguous elements, the voxel pairs
// (2 w', 2 w' + 1) of the input lines (2 d' + kd, 2 h' + kh), read where they lie.  Three kernels share that view:
//
//   pm_gemm<NT, false>  forward:        acc[n][m] += Wp[n][k] . A[m][k]      both operands K-contiguous in LDS
//   pm_gemm<NT, true>   data gradient:  acc[k][m] += Wp[n][k] . dY[m][n]     Wp tile read through transposing LDS reads
//   pm_wgrad<NT>        weight gradient: acc[n][k] += dY[m][n] . A[m][k]     both tiles read through transposing reads
//
// In all of them the MFMA "A" operand (result rows, 4 consecutive per lane and register quad) is the weight side and the
// "B" operand (result column = lane) the voxel side, so that a lane owns 4 consecutive channels of one voxel: 8-byte
// bf16 stores.  256 threads = 2 x 2 waves; a wave owns 64 voxels x 32 NT weight rows (NT = 3 when 2C is a multiple of
// 192, the Swin widths 96 / 192 / 384 / 768: the tile then spans 192 output channels and A is read once; NT = 1 otherwise).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/transoar_patchmerge.h"
#include "mfma_stream.hpp"

using namespace transoar;

namespace {

constexpr int kAbiVersion = 1;
constexpr int kCUs = 256;
constexpr int kBM = 128;                      // voxels (output rows) of a GEMM tile
constexpr int kBK = 64;                       // reduction elements per LDS stage
constexpr int kPitch = 2 * kBK + 16;          // bytes of a K-contiguous LDS row: 36 dwords, 8 x ds_read_b128 hit 32 banks once

struct Geo {
  int B, D, H, W, C;
  int Do, Ho, Wo, M;                          // output grid, M = B Do Ho Wo
};

// element offset of x[b, 2 d', 2 h', 2 w', 0] for output row m
__device__ __forceinline__ int row_base(const Geo& g, int m) {
  const int wo = m % g.Wo;
  int t = m / g.Wo;
  const int ho = t % g.Ho;
  t /= g.Ho;
  const int d_o = t % g.Do, b = t / g.Do;
  return (((b * g.D + 2 * d_o) * g.H + 2 * ho) * g.W + 2 * wo) * g.C;
}
// element offset, relative to row_base, of packed reduction index kk = (kd, kh, [kw, c])
__device__ __forceinline__ int k_offset(const Geo& g, int kk) {
  const int k2 = 2 * g.C;
  const int seg = (kk >= k2) + (kk >= 2 * k2) + (kk >= 3 * k2);
  return ((seg >> 1) * g.H + (seg & 1)) * g.W * g.C + (kk - seg * k2);
}

// fragment [32 columns (lane & 31)][16 rows 16 j + 8 kh .. + 7] of a row-major LDS tile: the transposing read of
// mfma_stream.hpp's frag_cols without its swizzle.  col_byte: byte offset of the 32-column block inside a row.
__device__ __forceinline__ s16x8 frag_tr(const unsigned char* tile, int pitch, int j, int col_byte, int lane) {
  const int kh = lane >> 5, gq = (lane >> 4) & 1, r = (lane & 15) >> 2, c = lane & 3;
  const unsigned char* p = tile + (16 * j + 8 * kh + r) * pitch + col_byte + 32 * gq + 8 * c;
  const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * pitch));
  return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---------------------------------------------------------------------------------------------------------------------
// weight pack: (2C, C, 2, 2, 2) fp32 / bf16 -> (2C, [tap, c]) bf16; one thread per (n, c) moves its 8 taps
template <typename T>
__global__ __launch_bounds__(256) void pm_pack(const T* __restrict__ w, unsigned short* __restrict__ packed, int C) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * C * C) return;
  const int n = idx / C, c = idx - n * C;
  float v[8];
  if constexpr (sizeof(T) == 4) {
    const float4 lo = *reinterpret_cast<const float4*>(w + (size_t)idx * 8), hi = *reinterpret_cast<const float4*>(w + (size_t)idx * 8 + 4);
    v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
  } else {
    const u32x4 q = *reinterpret_cast<const u32x4*>(w + (size_t)idx * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[2 * i] = bf16_lo(q[i]), v[2 * i + 1] = bf16_hi(q[i]);
  }
#pragma unroll
  for (int tap = 0; tap < 8; ++tap) packed[(size_t)n * 8 * C + tap * C + c] = static_cast<unsigned short>(pack_bf16(v[tap], 0.f) & 0xffffu);
}

// ---------------------------------------------------------------------------------------------------------------------
// forward (DGRAD false): act = x gathered by row_base + k_offset, reduction over 8C, result rows = output channels.
// data gradient (DGRAD true): act = dY (M x 2C, dense), reduction over 2C, result rows = packed index kk, stored to
//   dx at row_base + k_offset.
// grid (M tiles, N tiles, K splits); with K splits (forward only) fp32 partials go to `partial` (split, M, 2C).
template <int NT, bool DGRAD>
__global__ __launch_bounds__(256) void pm_gemm(const unsigned short* __restrict__ act, const unsigned short* __restrict__ wp,
                                               unsigned short* __restrict__ out, float* __restrict__ partial, Geo g,
                                               int chunks_per_split) {
  constexpr int BN = 64 * NT;
  constexpr int WROWS = DGRAD ? kBK : BN;
  constexpr int WPITCH = DGRAD ? 2 * BN + 16 : kPitch;
  constexpr int WPIECES = BN / 8;                       // 16-byte pieces of a weight tile row (DGRAD)
  __shared__ __attribute__((aligned(16))) unsigned char lds_a[kBM * kPitch];
  __shared__ __attribute__((aligned(16))) unsigned char lds_w[WROWS * WPITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 5, l31 = lane & 31;
  const int wm = wave & 1, wn = wave >> 1;
  const int k8 = 8 * g.C, co = 2 * g.C;
  const int ktot = DGRAD ? co : k8, nout = DGRAD ? k8 : co;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;
  const int n_chunks = (ktot + kBK - 1) / kBK;
  const int c_begin = blockIdx.z * chunks_per_split;
  const int c_end = min(n_chunks, c_begin + chunks_per_split);

  // what this thread stages: act rows (tid >> 3) + 32 i, piece tid & 7; weight pieces tid + 256 i
  const int pc = tid & 7;
  int a_ofs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = min(m0 + (tid >> 3) + 32 * i, g.M - 1);               // rows past the end: a valid row, never stored
    a_ofs[i] = DGRAD ? m * co : row_base(g, m);
  }
  int w_ofs[2 * NT];
#pragma unroll
  for (int i = 0; i < 2 * NT; ++i) {
    if constexpr (DGRAD) {
      const int id = tid + 256 * i;
      w_ofs[i] = min(n0 + (id % WPIECES) * 8, k8 - 8);                  // column of the piece; row = reduction index
    } else {
      w_ofs[i] = min(n0 + (tid >> 3) + 32 * i, nout - 1) * k8;
    }
  }

  u32x4 ra[4], rw[2 * NT];
  auto fetch = [&](int chunk) {
    const int kk = chunk * kBK + pc * 8;
    const bool ok = kk < ktot;
    const int kofs = DGRAD ? kk : k_offset(g, min(kk, ktot - 8));
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = ok ? *reinterpret_cast<const u32x4*>(act + a_ofs[i] + kofs) : u32x4{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      if constexpr (DGRAD) {
        const int n = chunk * kBK + (tid + 256 * i) / WPIECES;
        rw[i] = n < co ? *reinterpret_cast<const u32x4*>(wp + (size_t)n * k8 + w_ofs[i]) : u32x4{0, 0, 0, 0};
      } else {
        rw[i] = ok ? *reinterpret_cast<const u32x4*>(wp + w_ofs[i] + kk) : u32x4{0, 0, 0, 0};
      }
    }
  };

  f32x16 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;

  if (c_begin < c_end) fetch(c_begin);
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(lds_a + ((tid >> 3) + 32 * i) * kPitch + pc * 16) = ra[i];
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      if constexpr (DGRAD) {
        const int id = tid + 256 * i;
        *reinterpret_cast<u32x4*>(lds_w + (id / WPIECES) * WPITCH + (id % WPIECES) * 16) = rw[i];
      } else {
        *reinterpret_cast<u32x4*>(lds_w + ((tid >> 3) + 32 * i) * kPitch + pc * 16) = rw[i];
      }
    }
    __syncthreads();
    if (chunk + 1 < c_end) fetch(chunk + 1);                            // in flight under this stage's MFMAs
#pragma unroll
    for (int ks = 0; ks < kBK / 16; ++ks) {
      s16x8 fa[2], fw[NT];
#pragma unroll
      for (int u = 0; u < 2; ++u)
        fa[u] = *reinterpret_cast<const s16x8*>(lds_a + (wm * 64 + 32 * u + l31) * kPitch + ks * 32 + kh * 16);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if constexpr (DGRAD)
          fw[t] = frag_tr(lds_w, WPITCH, ks, (wn * 32 * NT + 32 * t) * 2, lane);
        else
          fw[t] = *reinterpret_cast<const s16x8*>(lds_w + (wn * 32 * NT + 32 * t + l31) * kPitch + ks * 32 + kh * 16);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = mfma(fw[t], fa[u], acc[t][u]);
    }
    __syncthreads();
  }

  // acc[t][u][e]: result row (weight side) nb + (e & 3) + 8 (e >> 2) + 4 kh, voxel m0 + 64 wm + 32 u + (lane & 31)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int m = m0 + wm * 64 + 32 * u + l31;
    if (m >= g.M) continue;
    const int o_row = DGRAD ? row_base(g, m) : m * co;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nb = n0 + wn * 32 * NT + 32 * t;                        // a block of 32 never straddles a K segment
      if (nb >= nout) continue;
      const int o_col = DGRAD ? k_offset(g, nb) : nb;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = 8 * q + 4 * kh;
        const float v0 = acc[t][u][4 * q], v1 = acc[t][u][4 * q + 1], v2 = acc[t][u][4 * q + 2], v3 = acc[t][u][4 * q + 3];
        if (!DGRAD && partial != nullptr)
          *reinterpret_cast<float4*>(partial + ((size_t)blockIdx.z * g.M + m) * co + nb + col) = make_float4(v0, v1, v2, v3);
        else
          *reinterpret_cast<u32x2*>(out + o_row + o_col + col) = u32x2{pack_bf16(v0, v1), pack_bf16(v2, v3)};
      }
    }
  }
}

// forward split-K combine: y = bf16(sum over splits, in order); one thread per 4 channels
__global__ __launch_bounds__(256) void pm_combine(const float* __restrict__ partial, unsigned short* __restrict__ y, int quads, int splits) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= quads) return;
  float4 s = reinterpret_cast<const float4*>(partial)[idx];
  for (int z = 1; z < splits; ++z) {
    const float4 p = reinterpret_cast<const float4*>(partial)[(size_t)z * quads + idx];
    s.x += p.x, s.y += p.y, s.z += p.z, s.w += p.w;
  }
  reinterpret_cast<u32x2*>(y)[idx] = u32x2{pack_bf16(s.x, s.y), pack_bf16(s.z, s.w)};
}

// zeros for the voxels of dx that no output voxel reads (the last plane / row / column of an odd extent); one thread per
// 16-byte piece of the map
__global__ __launch_bounds__(256) void pm_zero_dropped(unsigned short* __restrict__ dx, Geo g, int pieces) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= pieces) return;
  const int vox = idx / (g.C / 8);
  const int w = vox % g.W, h = (vox / g.W) % g.H, d = (vox / (g.W * g.H)) % g.D;
  if (w >= 2 * g.Wo || h >= 2 * g.Ho || d >= 2 * g.Do) reinterpret_cast<u32x4*>(dx)[idx] = u32x4{0, 0, 0, 0};
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient: workgroup (kk tile of 128, n tile of 64 NT, group of lines) accumulates dY^T . A over its output rows
// in steps of 32 rows; both tiles lie in LDS as they lie in memory (row = voxel) and are read transposed.
// partial (split, 2C, 8C) fp32.
template <int NT>
__global__ __launch_bounds__(256) void pm_wgrad(const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
                                                float* __restrict__ partial, Geo g, int rows_per_split) {
  constexpr int TN = 64 * NT, TK = 128;
  constexpr int DPITCH = 2 * TN + 16, XPITCH = 2 * TK + 16, DPIECES = TN / 8;
  __shared__ __attribute__((aligned(16))) unsigned char lds_d[32 * DPITCH];
  __shared__ __attribute__((aligned(16))) unsigned char lds_x[32 * XPITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 5, l31 = lane & 31;
  const int wn = wave & 1, wk = wave >> 1;
  const int k8 = 8 * g.C, co = 2 * g.C;
  const int kk0 = blockIdx.x * TK, n0 = blockIdx.y * TN;
  const int m_begin = blockIdx.z * rows_per_split, m_end = min(g.M, m_begin + rows_per_split);

  const int x_col = k_offset(g, kk0 + (tid & 15) * 8);                   // 8C is a multiple of 128: always inside
  u32x4 rx[2], rd[NT];
  auto fetch = [&](int mc) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mc + (tid >> 4) + 16 * i;
      rx[i] = m < m_end ? *reinterpret_cast<const u32x4*>(x + row_base(g, m) + x_col) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int id = tid + 256 * i;
      const int m = mc + id / DPIECES, n = n0 + (id % DPIECES) * 8;
      rd[i] = (m < m_end && n < co) ? *reinterpret_cast<const u32x4*>(dy + (size_t)m * co + n) : u32x4{0, 0, 0, 0};
    }
  };

  f32x16 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;

  if (m_begin < m_end) fetch(m_begin);
  for (int mc = m_begin; mc < m_end; mc += 32) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(lds_x + ((tid >> 4) + 16 * i) * XPITCH + (tid & 15) * 16) = rx[i];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int id = tid + 256 * i;
      *reinterpret_cast<u32x4*>(lds_d + (id / DPIECES) * DPITCH + (id % DPIECES) * 16) = rd[i];
    }
    __syncthreads();
    if (mc + 32 < m_end) fetch(mc + 32);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      s16x8 fd[NT], fx[2];
#pragma unroll
      for (int t = 0; t < NT; ++t) fd[t] = frag_tr(lds_d, DPITCH, j, (wn * 32 * NT + 32 * t) * 2, lane);
#pragma unroll
      for (int u = 0; u < 2; ++u) fx[u] = frag_tr(lds_x, XPITCH, j, (wk * 64 + 32 * u) * 2, lane);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = mfma(fd[t], fx[u], acc[t][u]);
    }
    __syncthreads();
  }

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int nb = n0 + wn * 32 * NT + 32 * t;
    if (nb >= co) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kk = kk0 + wk * 64 + 32 * u + l31;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = nb + (e & 3) + 8 * (e >> 2) + 4 * kh;
        partial[((size_t)blockIdx.z * co + n) * k8 + kk] = acc[t][u][e];
      }
    }
  }
}

// d_weight[n, c, tap] = sum over the groups of lines, in order, of partial[z, n, tap C + c]: the parameter layout in fp32
__global__ __launch_bounds__(256) void pm_wgrad_reduce(const float* __restrict__ partial, float* __restrict__ dw, int C, int splits) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int k8 = 8 * C, co = 2 * C;
  if (idx >= co * k8) return;
  const int n = idx / k8, rem = idx - n * k8, c = rem >> 3, tap = rem & 7;
  const size_t at = (size_t)n * k8 + tap * C + c;
  float s = partial[at];
  for (int z = 1; z < splits; ++z) s += partial[(size_t)z * co * k8 + at];
  dw[idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

int make_geo(int B, int D, int H, int W, int C, Geo* g) {
  if (B < 1 || D < 2 || H < 2 || W < 2 || C < 16 || C % 16 != 0 || C >= 8192) return TRANSOAR_PATCHMERGE_ERR_DIM;
  const long long x_bytes = 2ll * B * D * H * W * C;
  if (x_bytes >= (1ll << 31)) return TRANSOAR_PATCHMERGE_ERR_DIM;
  *g = Geo{B, D, H, W, C, D / 2, H / 2, W / 2, B * (D / 2) * (H / 2) * (W / 2)};
  return 0;
}
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline int nt_of(int C) { return (2 * C) % 192 == 0 ? 3 : 1; }
inline int cdiv(long long a, long long b) { return static_cast<int>((a + b - 1) / b); }

// forward: K splits so that the grid reaches about one workgroup per CU; 1 = bf16 straight from the GEMM
void forward_split(const Geo& g, int* splits, int* chunks_per_split) {
  const int tiles = cdiv(g.M, kBM) * cdiv(2 * g.C, 64 * nt_of(g.C));
  const int n_chunks = 8 * g.C / kBK;
  int s = tiles >= kCUs / 2 ? 1 : kCUs / tiles;
  if (s > n_chunks) s = n_chunks;
  *chunks_per_split = cdiv(n_chunks, s);
  *splits = cdiv(n_chunks, *chunks_per_split);
}
// weight gradient: groups of lines (multiples of 32 output rows) so that the grid reaches about two workgroups per CU
void wgrad_split(const Geo& g, int* splits, int* rows_per_split) {
  const int tiles = (8 * g.C / 128) * cdiv(2 * g.C, 64 * nt_of(g.C));
  int s = 2 * kCUs / tiles;
  if (s < 1) s = 1;
  const int steps = cdiv(g.M, 32);
  if (s > steps) s = steps;
  *rows_per_split = 32 * cdiv(steps, s);
  *splits = cdiv(g.M, *rows_per_split);
}

}  // namespace

extern "C" {

int transoar_patchmerge_abi_version(void) { return kAbiVersion; }

size_t transoar_patch_merge_workspace_bytes(int what, int B, int D, int H, int W, int C) {
  Geo g;
  if (make_geo(B, D, H, W, C, &g) != 0) return 0;
  int s, per;
  if (what == 0) {
    forward_split(g, &s, &per);
    return s > 1 ? (size_t)s * g.M * 2 * C * sizeof(float) : 16;
  }
  wgrad_split(g, &s, &per);
  return (size_t)s * 16 * C * C * sizeof(float);
}

int transoar_patch_merge_pack(const void* weight, int weight_dtype, void* packed, int C, void* hip_stream) {
  if (weight == nullptr || packed == nullptr) return TRANSOAR_PATCHMERGE_ERR_NULL;
  if (C < 16 || C % 16 != 0 || C >= 8192) return TRANSOAR_PATCHMERGE_ERR_DIM;
  if (weight_dtype != 0 && weight_dtype != 2) return TRANSOAR_PATCHMERGE_ERR_DTYPE;
  if (misaligned(weight) || misaligned(packed)) return TRANSOAR_PATCHMERGE_ERR_ALIGN;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int blocks = cdiv(2ll * C * C, 256);
  if (weight_dtype == 0)
    pm_pack<float><<<blocks, 256, 0, stream>>>(static_cast<const float*>(weight), static_cast<unsigned short*>(packed), C);
  else
    pm_pack<unsigned short><<<blocks, 256, 0, stream>>>(static_cast<const unsigned short*>(weight), static_cast<unsigned short*>(packed), C);
  return hipGetLastError();
}

int transoar_patch_merge_forward(const void* x, const void* packed, void* y, void* workspace, size_t workspace_bytes,
                                 int B, int D, int H, int W, int C, void* hip_stream) {
  if (x == nullptr || packed == nullptr || y == nullptr) return TRANSOAR_PATCHMERGE_ERR_NULL;
  Geo g;
  if (int rc = make_geo(B, D, H, W, C, &g)) return rc;
  if (misaligned(x) || misaligned(packed) || misaligned(y) || misaligned(workspace)) return TRANSOAR_PATCHMERGE_ERR_ALIGN;
  int splits, per;
  forward_split(g, &splits, &per);
  if (splits > 1 && (workspace == nullptr || workspace_bytes < (size_t)splits * g.M * 2 * C * sizeof(float)))
    return TRANSOAR_PATCHMERGE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int nt = nt_of(C);
  const dim3 grid(cdiv(g.M, kBM), cdiv(2 * C, 64 * nt), splits);
  const auto* xs = static_cast<const unsigned short*>(x);
  const auto* ws = static_cast<const unsigned short*>(packed);
  auto* ys = static_cast<unsigned short*>(y);
  float* part = splits > 1 ? static_cast<float*>(workspace) : nullptr;
  if (nt == 3)
    pm_gemm<3, false><<<grid, 256, 0, stream>>>(xs, ws, ys, part, g, per);
  else
    pm_gemm<1, false><<<grid, 256, 0, stream>>>(xs, ws, ys, part, g, per);
  if (splits > 1) {
    const int quads = g.M * 2 * C / 4;
    pm_combine<<<cdiv(quads, 256), 256, 0, stream>>>(part, ys, quads, splits);
  }
  return hipGetLastError();
}

int transoar_patch_merge_dgrad(const void* dy, const void* packed, void* dx, int B, int D, int H, int W, int C,
                               void* hip_stream) {
  if (dy == nullptr || packed == nullptr || dx == nullptr) return TRANSOAR_PATCHMERGE_ERR_NULL;
  Geo g;
  if (int rc = make_geo(B, D, H, W, C, &g)) return rc;
  if (misaligned(dy) || misaligned(packed) || misaligned(dx)) return TRANSOAR_PATCHMERGE_ERR_ALIGN;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int nt = nt_of(C);
  const dim3 grid(cdiv(g.M, kBM), cdiv(8 * C, 64 * nt), 1);
  const auto* ds = static_cast<const unsigned short*>(dy);
  const auto* ws = static_cast<const unsigned short*>(packed);
  auto* xs = static_cast<unsigned short*>(dx);
  const int per = cdiv(2 * C, kBK);
  if ((D | H | W) & 1) {
    const int pieces = B * D * H * W * (C / 8);
    pm_zero_dropped<<<cdiv(pieces, 256), 256, 0, stream>>>(xs, g, pieces);
  }
  if (nt == 3)
    pm_gemm<3, true><<<grid, 256, 0, stream>>>(ds, ws, xs, nullptr, g, per);
  else
    pm_gemm<1, true><<<grid, 256, 0, stream>>>(ds, ws, xs, nullptr, g, per);
  return hipGetLastError();
}

int transoar_patch_merge_wgrad(const void* x, const void* dy, float* d_weight, void* workspace, size_t workspace_bytes,
                               int B, int D, int H, int W, int C, void* hip_stream) {
  if (x == nullptr || dy == nullptr || d_weight == nullptr || workspace == nullptr) return TRANSOAR_PATCHMERGE_ERR_NULL;
  Geo g;
  if (int rc = make_geo(B, D, H, W, C, &g)) return rc;
  if (misaligned(x) || misaligned(dy) || misaligned(d_weight) || misaligned(workspace)) return TRANSOAR_PATCHMERGE_ERR_ALIGN;
  int splits, per;
  wgrad_split(g, &splits, &per);
  if (workspace_bytes < (size_t)splits * 16 * C * C * sizeof(float)) return TRANSOAR_PATCHMERGE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int nt = nt_of(C);
  const dim3 grid(8 * C / 128, cdiv(2 * C, 64 * nt), splits);
  const auto* xs = static_cast<const unsigned short*>(x);
  const auto* ds = static_cast<const unsigned short*>(dy);
  float* part = static_cast<float*>(workspace);
  if (nt == 3)
    pm_wgrad<3><<<grid, 256, 0, stream>>>(xs, ds, part, g, per);
  else
    pm_wgrad<1><<<grid, 256, 0, stream>>>(xs, ds, part, g, per);
  pm_wgrad_reduce<<<cdiv(16ll * C * C, 256), 256, 0, stream>>>(part, d_weight, C, splits);
  return hipGetLastError();
}

}  // extern "C"
