// Dense multi-head cross-attention of the Focused Decoder at head dimension 48 (gfx950): flash attention over
// (B, N, 384) bf16 token matrices whose heads are read and written IN PLACE as 48-column slices.
//
// Reference semantics: FocusedAttn.forward, transoar/models/necks/focused_decoder.py:228-262, for the cases the RoI
// gather (csrc/attn.hip) does not take: restrict_attn False, or attention volumes too large to gather.  Per (b, h):
//
//     O = softmax_rows(mask(scale Q_h K_h^T)) V_h          Q_h (Nq x 48), K_h / V_h (L x 48), L = 12 800 .. 16 384
//
// Four kernels and two small combine passes:
//   dense_attn_fwd      grid (n_split, ceil(Nq / 64), B H)   QK^T -> mask -> online softmax -> PV, lse saved
//   dense_attn_delta    rowsum(dO o O) per (b, h, row)
//   dense_attn_bwd_q    grid (n_split, ceil(Nq / 64), B H)   recomputes P from lse; dQ
//   dense_attn_bwd_kv   grid (ceil(L / 64), B H)             owns 64 keys, loops over the queries; dK and dV (no atomics)
//
// Common structure, shaped by hd = 48 = 3 x 16:
//   * 256 threads = 4 waves; a wave owns 16 stationary rows (queries in fwd / bwd_q, keys in bwd_kv) whose 48 channels
//     are three B fragments of v_mfma_f32_16x16x16_bf16 (4 bf16 per lane: 2 registers each), read straight from HBM;
//   * the streamed operand comes in stages of 64 rows x 96 bytes.  Every product is computed TRANSPOSED, with the
//     streamed tile as the A operand and the stationary rows as the columns: S^T = K Q^T puts the 4 results of a lane
//     at (keys 4 g .. 4 g + 3, query lane % 16), which is exactly the B fragment layout of the next product
//     (O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T P, dK^T += Q^T dS): P and dS go back into the matrix cores after a
//     bf16 pack, with no shuffle and no LDS round trip, and a row's softmax state lives in the 4 lanes that share
//     lane % 16 (two exchanges per reduction);
//   * the second product needs the streamed tile with its rows along K, i.e. transposed.  The stage is therefore
//     fetched into registers (16 bytes per thread and piece, issued one whole stage ahead of its use), and written to
//     LDS twice where both forms are needed: row-major (112-byte rows: 16-byte aligned, 28-bank stride) and transposed
//     ([48][68] bf16).  An LDS-DMA cannot produce the transposed image, and at 12 MFMAs per wave and 32 keys the
//     interval is too short for a DMA ring to pay (section 11.3): two LDS stages, one barrier per 64 rows;
//   * softmax state in fp32 registers, base-2 exponentials (scale log2(e) folded into one multiply); the mask word of a
//     32-key tile is read once per lane (a 64-row block may span several organs), and a tile whose word is all ones
//     for every lane of a wave is skipped by that wave; whole stages outside the organs' [first, last) live tiles are
//     never loaded.
// Registers: 6 (stationary fragments; 12 in the backward kernels) + 12 (accumulator; 24 in bwd_kv) + 8 scores + 4
// staged pieces x 4 -- under 100 per lane, so several workgroups share a CU and hide each other's barriers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/transoar_denseattn.h"

#include "mfma_stream.hpp"

namespace transoar {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDC = 384;                  // channels of a token
constexpr int kDH = 8;                    // heads
constexpr int kHd = 48;                   // channels of a head
constexpr int kStage = 64;                // streamed rows per LDS stage (two 32-key mask tiles)
constexpr int kRowStride = 56;            // shorts per row of the row-major image (48 + 8 padding)
constexpr int kColStride = 68;            // shorts per channel of the transposed image (64 + 4 padding)
constexpr int kRowImage = kStage * kRowStride;        // 3584 shorts
constexpr int kColImage = kHd * kColStride;           // 3264 shorts

__device__ __forceinline__ f32x4 mfma16(s16x4 a, s16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ s16x4 pack4(float a, float b, float c, float d) {
  return __builtin_bit_cast(s16x4, u32x2{pack_bf16(a, b), pack_bf16(c, d)});
}
__device__ __forceinline__ float quad_max(float v) {          // over the 4 lanes that share lane % 16
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
// mask bits of the keys >= L in 32-key tile t
__device__ __forceinline__ unsigned tail_word(int t, int L) {
  const int valid = L - 32 * t;
  return valid >= 32 ? 0u : (valid <= 0 ? ~0u : (~0u << valid));
}
// the mask word of tile t for the organ whose words start at bits_row (nullptr: nothing but the tail is masked)
__device__ __forceinline__ unsigned mask_word(const unsigned* bits_row, int t, int n_tiles, int L) {
  if (t >= n_tiles) return ~0u;
  unsigned w = tail_word(t, L);
  if (bits_row != nullptr) w |= bits_row[t];
  return w;
}

// One stage of a head slice in registers: the 384 16-byte pieces of 64 rows x 96 bytes, piece tid and piece tid + 256.
// Rows past the end of the matrix repeat its last row (finite data; whoever consumes them masks their contribution).
struct Pieces {
  u32x4 p[2];
};
__device__ __forceinline__ Pieces load_slice(const unsigned short* __restrict__ head_base, int row0, int n_rows, int tid) {
  Pieces s;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    s.p[i] = u32x4{0u, 0u, 0u, 0u};
    if (id < kStage * 6) {
      const int r = id / 6, pc = id - 6 * r;
      const int row = min(row0 + r, n_rows - 1);
      s.p[i] = *reinterpret_cast<const u32x4*>(head_base + static_cast<long>(row) * kDC + 8 * pc);
    }
  }
  return s;
}
__device__ __forceinline__ void store_rows(unsigned short* image, const Pieces& s, int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    if (id < kStage * 6) {
      const int r = id / 6, pc = id - 6 * r;
      *reinterpret_cast<u32x4*>(image + r * kRowStride + 8 * pc) = s.p[i];
    }
  }
}
__device__ __forceinline__ void store_cols(unsigned short* image, const Pieces& s, int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    if (id < kStage * 6) {
      const int r = id / 6, pc = id - 6 * r;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        image[(8 * pc + 2 * e) * kColStride + r] = static_cast<unsigned short>(s.p[i][e] & 0xffffu);
        image[(8 * pc + 2 * e + 1) * kColStride + r] = static_cast<unsigned short>(s.p[i][e] >> 16);
      }
    }
  }
}
// A fragment of the row-major image: rows r0 + lane % 16, channels 16 ks + 4 g .. + 3
__device__ __forceinline__ s16x4 frag_row(const unsigned short* image, int r0, int ks, int c, int g) {
  return *reinterpret_cast<const s16x4*>(image + (r0 + c) * kRowStride + 16 * ks + 4 * g);
}
// A fragment of the transposed image: channels 16 ct + lane % 16, rows r0 + 4 g .. + 3
__device__ __forceinline__ s16x4 frag_col(const unsigned short* image, int ct, int r0, int c, int g) {
  return *reinterpret_cast<const s16x4*>(image + (16 * ct + c) * kColStride + r0 + 4 * g);
}
// the three stationary B fragments of a row: channels 16 ks + 4 g .. + 3
__device__ __forceinline__ void load_row48(const unsigned short* __restrict__ row_ptr, int g, s16x4 (&f)[3]) {
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) f[ks] = *reinterpret_cast<const s16x4*>(row_ptr + 16 * ks + 4 * g);
}

// stages [s0, s1) of 64 keys this workgroup streams: the live tiles of the block's organs, divided among the splits
__device__ __forceinline__ void key_stages(const int* __restrict__ bounds, int r0, int Nq, int rpo, int n_tiles, int n_split,
                                           int split, int& s0, int& s1) {
  int t_lo = 0, t_hi = n_tiles;
  if (bounds != nullptr) {
    const int o_lo = r0 / rpo, o_hi = min(r0 + kStage - 1, Nq - 1) / rpo;
    t_lo = n_tiles;
    t_hi = 0;
    for (int o = o_lo; o <= o_hi; ++o) {
      t_lo = min(t_lo, bounds[2 * o]);
      t_hi = max(t_hi, bounds[2 * o + 1]);
    }
    t_lo = max(t_lo, 0);
    t_hi = min(t_hi, n_tiles);
  }
  const int s_lo = t_lo / 2, s_hi = max((t_hi + 1) / 2, s_lo);
  const int chunk = (s_hi - s_lo + n_split - 1) / n_split;
  s0 = min(s_lo + split * chunk, s_hi);
  s1 = min(s0 + chunk, s_hi);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dense_attn_fwd(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned* __restrict__ keybits, const int* __restrict__ bounds, unsigned short* __restrict__ out,
    float* __restrict__ lse, float* __restrict__ pacc, float* __restrict__ pm, float* __restrict__ pl, int Nq, int L,
    int rpo, int bits_stride, float scale_log2, int n_split) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[2][kRowImage + kColImage];
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int split = blockIdx.x, r0 = blockIdx.y * kStage, bh = blockIdx.z;
  const int b = bh / kDH, h = bh - b * kDH;
  const int row = r0 + wave * 16 + c, rowc = min(row, Nq - 1);
  const int n_tiles = (L + 31) / 32;
  const unsigned short* kbase = k + static_cast<long>(b) * L * kDC + kHd * h;
  const unsigned short* vbase = v + static_cast<long>(b) * L * kDC + kHd * h;
  const unsigned* bits_row = keybits == nullptr ? nullptr : keybits + static_cast<long>(rowc / rpo) * bits_stride;
  int s0, s1;
  key_stages(bounds, r0, Nq, rpo, n_tiles, n_split, split, s0, s1);

  s16x4 qf[3];
  load_row48(q + (static_cast<long>(b) * Nq + rowc) * kDC + kHd * h, g, qf);
  f32x4 acc[3];
#pragma unroll
  for (int ct = 0; ct < 3; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;             // running maximum (log2 units), this lane's part of the running sum

  if (s0 < s1) {
    store_rows(lds[0], load_slice(kbase, s0 * kStage, L, tid), tid);
    store_cols(lds[0] + kRowImage, load_slice(vbase, s0 * kStage, L, tid), tid);
  }
  __syncthreads();
  for (int s = s0; s < s1; ++s) {
    const int cur = (s - s0) & 1;
    const unsigned short* k_img = lds[cur];
    const unsigned short* vt_img = lds[cur] + kRowImage;
    Pieces nk, nv;
    if (s + 1 < s1) {
      nk = load_slice(kbase, (s + 1) * kStage, L, tid);
      nv = load_slice(vbase, (s + 1) * kStage, L, tid);
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const unsigned word = mask_word(bits_row, 2 * s + tt, n_tiles, L);
      if (__all(word == ~0u)) continue;             // no lane of this wave has a live key in the tile
      // ---- S^T[key][query] = K Q^T
      f32x4 sc[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) sc[kt] = mfma16(frag_row(k_img, 32 * tt + 16 * kt, ks, c, g), qf[ks], sc[kt]);
      }
      // ---- mask, online softmax (log2 units)
      float s2[2][4];
      float mt = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool masked = (word >> (16 * kt + 4 * g + e)) & 1u;
          s2[kt][e] = masked ? -INFINITY : sc[kt][e] * scale_log2;
          mt = fmaxf(mt, s2[kt][e]);
        }
      const float m_new = fmaxf(m_run, quad_max(mt));
      const float alpha = m_new == -INFINITY ? 1.f : fast_exp2(m_run - m_new);       // m_run = -inf: 0, and acc is 0
#pragma unroll
      for (int ct = 0; ct < 3; ++ct) acc[ct] *= alpha;
      l_run *= alpha;
      m_run = m_new;
      const float m_use = m_run == -INFINITY ? 0.f : m_run;
      s16x4 pf[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        float p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          p[e] = fast_exp2(s2[kt][e] - m_use);
          l_run += p[e];
        }
        pf[kt] = pack4(p[0], p[1], p[2], p[3]);
      }
      // ---- O^T[channel][query] += V^T P^T
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int ct = 0; ct < 3; ++ct) acc[ct] = mfma16(frag_col(vt_img, ct, 32 * tt + 16 * kt, c, g), pf[kt], acc[ct]);
    }
    if (s + 1 < s1) {
      store_rows(lds[cur ^ 1], nk, tid);
      store_cols(lds[cur ^ 1] + kRowImage, nv, tid);
    }
    __syncthreads();
  }

  const float l_tot = quad_sum(l_run);
  if (row >= Nq) return;
  if (n_split == 1) {
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    unsigned short* dst = out + (static_cast<long>(b) * Nq + row) * kDC + kHd * h + 4 * g;
#pragma unroll
    for (int ct = 0; ct < 3; ++ct)
      *reinterpret_cast<s16x4*>(dst + 16 * ct) = pack4(acc[ct][0] * inv, acc[ct][1] * inv, acc[ct][2] * inv, acc[ct][3] * inv);
    if (g == 0) lse[static_cast<long>(bh) * Nq + row] = (m_run + log2f(l_tot)) * kLn2;
  } else {
    const long prow = (static_cast<long>(bh) * n_split + split) * Nq + row;
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) *reinterpret_cast<f32x4*>(pacc + prow * kHd + 16 * ct + 4 * g) = acc[ct];
    if (g == 0) {
      pm[prow] = m_run;
      pl[prow] = l_tot;
    }
  }
}

// merge the splits' partial results: one thread per (b, h, row, 4 channels)
__global__ __launch_bounds__(256) void dense_attn_fwd_combine(const float* __restrict__ pacc, const float* __restrict__ pm,
                                                              const float* __restrict__ pl, unsigned short* __restrict__ out,
                                                              float* __restrict__ lse, int Nq, int n_split, long items) {
  const long id = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (id >= items) return;
  const long hrow = id / 12;                          // (b H + h) Nq + row
  const int cg = static_cast<int>(id - hrow * 12);
  const long bh = hrow / Nq;
  const int row = static_cast<int>(hrow - bh * Nq);
  const long p0 = bh * n_split * Nq + row;
  float m = -INFINITY;
  for (int s = 0; s < n_split; ++s) m = fmaxf(m, pm[p0 + static_cast<long>(s) * Nq]);
  const float m_use = m == -INFINITY ? 0.f : m;
  float l = 0.f;
  f32x4 acc{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < n_split; ++s) {
    const long prow = p0 + static_cast<long>(s) * Nq;
    const float w = fast_exp2(pm[prow] - m_use);
    l += w * pl[prow];
    acc += w * *reinterpret_cast<const f32x4*>(pacc + prow * kHd + 4 * cg);
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  const long b = bh / kDH;
  const int h = static_cast<int>(bh - b * kDH);
  *reinterpret_cast<s16x4*>(out + (b * Nq + row) * kDC + kHd * h + 4 * cg) =
      pack4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
  if (cg == 0) lse[hrow] = (m + log2f(l)) * kLn2;
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// delta[b, h, row] = rowsum(dO o O) over the head's 48 channels: one thread per (b, row, h)
__global__ __launch_bounds__(256) void dense_attn_delta(const unsigned short* __restrict__ out, const unsigned short* __restrict__ d_out,
                                                        float* __restrict__ delta, int Nq, long items) {
  const long id = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (id >= items) return;
  const long brow = id / kDH;
  const int h = static_cast<int>(id - brow * kDH);
  const long b = brow / Nq;
  const int row = static_cast<int>(brow - b * Nq);
  const u32x4* po = reinterpret_cast<const u32x4*>(out + brow * kDC + kHd * h);
  const u32x4* pd = reinterpret_cast<const u32x4*>(d_out + brow * kDC + kHd * h);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const u32x4 a = po[i], d = pd[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) sum += bf16_lo(a[e]) * bf16_lo(d[e]) + bf16_hi(a[e]) * bf16_hi(d[e]);
  }
  delta[(b * kDH + h) * Nq + row] = sum;
}

// dQ: the forward's work split; P is recomputed from lse, dQ^T[channel][query] += K^T dS^T
__global__ __launch_bounds__(256) void dense_attn_bwd_q(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ d_out, const float* __restrict__ lse, const float* __restrict__ delta,
    const unsigned* __restrict__ keybits, const int* __restrict__ bounds, unsigned short* __restrict__ dq,
    float* __restrict__ pdq, int Nq, int L, int rpo, int bits_stride, float scale, int n_split) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[2][2 * kRowImage + kColImage];
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int split = blockIdx.x, r0 = blockIdx.y * kStage, bh = blockIdx.z;
  const int b = bh / kDH, h = bh - b * kDH;
  const int row = r0 + wave * 16 + c, rowc = min(row, Nq - 1);
  const int n_tiles = (L + 31) / 32;
  const float scale_log2 = scale * kLog2e;
  const unsigned short* kbase = k + static_cast<long>(b) * L * kDC + kHd * h;
  const unsigned short* vbase = v + static_cast<long>(b) * L * kDC + kHd * h;
  const unsigned* bits_row = keybits == nullptr ? nullptr : keybits + static_cast<long>(rowc / rpo) * bits_stride;
  int s0, s1;
  key_stages(bounds, r0, Nq, rpo, n_tiles, n_split, split, s0, s1);

  s16x4 qf[3], df[3];
  load_row48(q + (static_cast<long>(b) * Nq + rowc) * kDC + kHd * h, g, qf);
  load_row48(d_out + (static_cast<long>(b) * Nq + rowc) * kDC + kHd * h, g, df);
  const float lse2 = lse[static_cast<long>(bh) * Nq + rowc] * kLog2e;
  const float dl = delta[static_cast<long>(bh) * Nq + rowc];
  f32x4 acc[3];
#pragma unroll
  for (int ct = 0; ct < 3; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (s0 < s1) {
    const Pieces pk = load_slice(kbase, s0 * kStage, L, tid);
    store_rows(lds[0], pk, tid);
    store_cols(lds[0] + 2 * kRowImage, pk, tid);
    store_rows(lds[0] + kRowImage, load_slice(vbase, s0 * kStage, L, tid), tid);
  }
  __syncthreads();
  for (int s = s0; s < s1; ++s) {
    const int cur = (s - s0) & 1;
    const unsigned short* k_img = lds[cur];
    const unsigned short* v_img = lds[cur] + kRowImage;
    const unsigned short* kt_img = lds[cur] + 2 * kRowImage;
    Pieces nk, nv;
    if (s + 1 < s1) {
      nk = load_slice(kbase, (s + 1) * kStage, L, tid);
      nv = load_slice(vbase, (s + 1) * kStage, L, tid);
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const unsigned word = mask_word(bits_row, 2 * s + tt, n_tiles, L);
      if (__all(word == ~0u)) continue;
      s16x4 dsf[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f32x4 sc{0.f, 0.f, 0.f, 0.f}, dp{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
          sc = mfma16(frag_row(k_img, 32 * tt + 16 * kt, ks, c, g), qf[ks], sc);       // S^T = K Q^T
          dp = mfma16(frag_row(v_img, 32 * tt + 16 * kt, ks, c, g), df[ks], dp);       // dP^T = V dO^T
        }
        float ds[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool masked = (word >> (16 * kt + 4 * g + e)) & 1u;
          const float p = masked ? 0.f : fast_exp2(sc[e] * scale_log2 - lse2);
          ds[e] = p * (dp[e] - dl);
        }
        dsf[kt] = pack4(ds[0], ds[1], ds[2], ds[3]);
      }
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int ct = 0; ct < 3; ++ct) acc[ct] = mfma16(frag_col(kt_img, ct, 32 * tt + 16 * kt, c, g), dsf[kt], acc[ct]);
    }
    if (s + 1 < s1) {
      store_rows(lds[cur ^ 1], nk, tid);
      store_cols(lds[cur ^ 1] + 2 * kRowImage, nk, tid);
      store_rows(lds[cur ^ 1] + kRowImage, nv, tid);
    }
    __syncthreads();
  }

  if (row >= Nq) return;
  if (n_split == 1) {
    unsigned short* dst = dq + (static_cast<long>(b) * Nq + row) * kDC + kHd * h + 4 * g;
#pragma unroll
    for (int ct = 0; ct < 3; ++ct)
      *reinterpret_cast<s16x4*>(dst + 16 * ct) = pack4(acc[ct][0] * scale, acc[ct][1] * scale, acc[ct][2] * scale, acc[ct][3] * scale);
  } else {
    const long prow = (static_cast<long>(bh) * n_split + split) * Nq + row;
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) *reinterpret_cast<f32x4*>(pdq + prow * kHd + 16 * ct + 4 * g) = acc[ct];
  }
}

// dq = scale . sum of the splits' partials: one thread per (b, h, row, 4 channels)
__global__ __launch_bounds__(256) void dense_attn_dq_combine(const float* __restrict__ pdq, unsigned short* __restrict__ dq, int Nq,
                                                             int n_split, float scale, long items) {
  const long id = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (id >= items) return;
  const long hrow = id / 12;
  const int cg = static_cast<int>(id - hrow * 12);
  const long bh = hrow / Nq;
  const int row = static_cast<int>(hrow - bh * Nq);
  f32x4 acc{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < n_split; ++s)
    acc += *reinterpret_cast<const f32x4*>(pdq + ((bh * n_split + s) * Nq + row) * kHd + 4 * cg);
  const long b = bh / kDH;
  const int h = static_cast<int>(bh - b * kDH);
  *reinterpret_cast<s16x4*>(dq + (b * Nq + row) * kDC + kHd * h + 4 * cg) =
      pack4(acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale);
}

// dK / dV: the workgroup owns 64 keys (a wave 16 of them, stationary) and streams the queries in stages of 64 rows of
// Q and dO, each kept row-major (S = Q K^T, dP = dO V^T) and transposed (dV^T += dO^T P, dK^T += Q^T dS).
struct RowStats {          // per-stage values of the streamed queries, staged with them
  float lse2, delta;       // threads 0 .. 63: query tid
  unsigned word;           // threads 64 .. 191: query (tid - 64) / 2, mask word (tid - 64) % 2 of the block's two key tiles
};
__global__ __launch_bounds__(256) void dense_attn_bwd_kv(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
    const unsigned short* __restrict__ d_out, const float* __restrict__ lse, const float* __restrict__ delta,
    const unsigned* __restrict__ keybits, const int* __restrict__ bounds, unsigned short* __restrict__ dk,
    unsigned short* __restrict__ dv, int Nq, int L, int O, int rpo, int bits_stride, float scale) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[2][2 * kRowImage + 2 * kColImage];
  __shared__ __attribute__((aligned(16))) float lds_lse[2][kStage];
  __shared__ __attribute__((aligned(16))) float lds_delta[2][kStage];
  __shared__ unsigned lds_word[2][kStage][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int kb = blockIdx.x, bh = blockIdx.y;
  const int b = bh / kDH, h = bh - b * kDH;
  const int key = kb * kStage + wave * 16 + c, keyc = min(key, L - 1);
  const int n_tiles = (L + 31) / 32;
  const float scale_log2 = scale * kLog2e;
  const unsigned short* qbase = q + static_cast<long>(b) * Nq * kDC + kHd * h;
  const unsigned short* dbase = d_out + static_cast<long>(b) * Nq * kDC + kHd * h;
  const float* lse_h = lse + static_cast<long>(bh) * Nq;
  const float* delta_h = delta + static_cast<long>(bh) * Nq;

  // the queries that may see a key of this block: the rows of the organs whose live tiles reach it
  int q_lo = 0, q_hi = Nq;
  if (bounds != nullptr) {
    q_lo = Nq;
    q_hi = 0;
    for (int o = 0; o < O; ++o)
      if (bounds[2 * o] <= 2 * kb + 1 && bounds[2 * o + 1] > 2 * kb) {
        q_lo = min(q_lo, o * rpo);
        q_hi = max(q_hi, (o + 1) * rpo);
      }
    q_hi = min(q_hi, Nq);
  }
  const int s0 = q_lo / kStage, s1 = max((q_hi + kStage - 1) / kStage, s0);

  auto load_stats = [&](int s) {
    RowStats st{0.f, 0.f, ~0u};
    if (tid < kStage) {
      const int qr = s * kStage + tid;
      st.lse2 = qr < Nq ? lse_h[qr] * kLog2e : INFINITY;        // rows past Nq: P = exp2(S - inf) = 0
      st.delta = qr < Nq ? delta_h[qr] : 0.f;
    } else if (tid < 3 * kStage) {
      const int j = tid - kStage;
      const int qr = min(s * kStage + (j >> 1), Nq - 1);
      st.word = mask_word(keybits == nullptr ? nullptr : keybits + static_cast<long>(qr / rpo) * bits_stride, 2 * kb + (j & 1),
                          n_tiles, L);
    }
    return st;
  };
  auto store_stats = [&](int stage, const RowStats& st) {
    if (tid < kStage) {
      lds_lse[stage][tid] = st.lse2;
      lds_delta[stage][tid] = st.delta;
    } else if (tid < 3 * kStage) {
      const int j = tid - kStage;
      lds_word[stage][j >> 1][j & 1] = st.word;
    }
  };

  s16x4 kf[3], vf[3];
  load_row48(k + (static_cast<long>(b) * L + keyc) * kDC + kHd * h, g, kf);
  load_row48(v + (static_cast<long>(b) * L + keyc) * kDC + kHd * h, g, vf);
  f32x4 acc_k[3], acc_v[3];
#pragma unroll
  for (int ct = 0; ct < 3; ++ct) {
    acc_k[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_v[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  if (s0 < s1) {
    const Pieces pq = load_slice(qbase, s0 * kStage, Nq, tid), pd = load_slice(dbase, s0 * kStage, Nq, tid);
    store_rows(lds[0], pq, tid);
    store_rows(lds[0] + kRowImage, pd, tid);
    store_cols(lds[0] + 2 * kRowImage, pq, tid);
    store_cols(lds[0] + 2 * kRowImage + kColImage, pd, tid);
    store_stats(0, load_stats(s0));
  }
  __syncthreads();
  const int my_word = wave >> 1, my_bit = 16 * (wave & 1) + c;
  for (int s = s0; s < s1; ++s) {
    const int cur = (s - s0) & 1;
    const unsigned short* q_img = lds[cur];
    const unsigned short* d_img = lds[cur] + kRowImage;
    const unsigned short* qt_img = lds[cur] + 2 * kRowImage;
    const unsigned short* dt_img = lds[cur] + 2 * kRowImage + kColImage;
    Pieces nq, nd;
    RowStats ns{0.f, 0.f, ~0u};
    if (s + 1 < s1) {
      nq = load_slice(qbase, (s + 1) * kStage, Nq, tid);
      nd = load_slice(dbase, (s + 1) * kStage, Nq, tid);
      ns = load_stats(s + 1);
    }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const int ql = 16 * qt + 4 * g;                 // this lane's queries ql .. ql + 3 of the stage
      bool masked[4];
      bool all_masked = true;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        masked[e] = (lds_word[cur][ql + e][my_word] >> my_bit) & 1u;
        all_masked = all_masked && masked[e];
      }
      if (__all(all_masked)) continue;                // none of the wave's keys is live for these 16 queries
      f32x4 sc{0.f, 0.f, 0.f, 0.f}, dp{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        sc = mfma16(frag_row(q_img, 16 * qt, ks, c, g), kf[ks], sc);          // S[query][key] = Q K^T
        dp = mfma16(frag_row(d_img, 16 * qt, ks, c, g), vf[ks], dp);          // dP = dO V^T
      }
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(&lds_lse[cur][ql]);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(&lds_delta[cur][ql]);
      float p[4], ds[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = masked[e] ? 0.f : fast_exp2(sc[e] * scale_log2 - l4[e]);
        ds[e] = p[e] * (dp[e] - d4[e]);
      }
      const s16x4 pf = pack4(p[0], p[1], p[2], p[3]), dsf = pack4(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
      for (int ct = 0; ct < 3; ++ct) {
        acc_v[ct] = mfma16(frag_col(dt_img, ct, 16 * qt, c, g), pf, acc_v[ct]);       // dV^T += dO^T P
        acc_k[ct] = mfma16(frag_col(qt_img, ct, 16 * qt, c, g), dsf, acc_k[ct]);      // dK^T += Q^T dS
      }
    }
    if (s + 1 < s1) {
      store_rows(lds[cur ^ 1], nq, tid);
      store_rows(lds[cur ^ 1] + kRowImage, nd, tid);
      store_cols(lds[cur ^ 1] + 2 * kRowImage, nq, tid);
      store_cols(lds[cur ^ 1] + 2 * kRowImage + kColImage, nd, tid);
      store_stats(cur ^ 1, ns);
    }
    __syncthreads();
  }

  if (key >= L) return;
  const long off = (static_cast<long>(b) * L + key) * kDC + kHd * h + 4 * g;
#pragma unroll
  for (int ct = 0; ct < 3; ++ct) {
    *reinterpret_cast<s16x4*>(dk + off + 16 * ct) =
        pack4(acc_k[ct][0] * scale, acc_k[ct][1] * scale, acc_k[ct][2] * scale, acc_k[ct][3] * scale);
    *reinterpret_cast<s16x4*>(dv + off + 16 * ct) = pack4(acc_v[ct][0], acc_v[ct][1], acc_v[ct][2], acc_v[ct][3]);
  }
}

namespace {

constexpr long kMaxBytes = (1L << 31) - 1;

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// everything that does not depend on the pointers: 0 or a negative code
int check_dims(int B, int Nq, long L, int C, int H, int O, int rows_per_organ, bool has_bits, int n_split) {
  if (C != kDC || H != kDH || B < 1 || Nq < 1 || L < 1 || n_split < 1 || n_split > 64) return TRANSOAR_DENSEATTN_ERR_DIM;
  if (static_cast<long>(B) * H > 65535) return TRANSOAR_DENSEATTN_ERR_DIM;
  if (static_cast<long>(B) * Nq * kDC * 2 > kMaxBytes || static_cast<long>(B) * L * kDC * 2 > kMaxBytes)
    return TRANSOAR_DENSEATTN_ERR_DIM;
  if (transoar_dense_attn_workspace_bytes(B, Nq, n_split) > static_cast<size_t>(kMaxBytes)) return TRANSOAR_DENSEATTN_ERR_DIM;
  if (has_bits) {
    if (O < 1 || rows_per_organ < 1 || static_cast<long>(O) * rows_per_organ != Nq) return TRANSOAR_DENSEATTN_ERR_DIM;
    if (static_cast<long>(O) * ((L + 31) / 32) * 4 > kMaxBytes) return TRANSOAR_DENSEATTN_ERR_DIM;
  }
  return 0;
}

struct Workspace {
  float *delta, *pacc, *pm, *pl;
};
Workspace carve(void* workspace, int B, int Nq, int n_split) {
  const long rows = static_cast<long>(B) * kDH * Nq;
  Workspace w;
  w.delta = static_cast<float*>(workspace);
  w.pacc = w.delta + rows;
  w.pm = w.pacc + rows * n_split * kHd;
  w.pl = w.pm + rows * n_split;
  return w;
}

}  // namespace
}  // namespace transoar

using namespace transoar;

extern "C" size_t transoar_dense_attn_workspace_bytes(int B, int Nq, int n_split) {
  if (B < 1 || Nq < 1 || n_split < 1) return 0;
  const size_t rows = static_cast<size_t>(B) * kDH * Nq;
  return rows * 4 * (1 + (n_split > 1 ? static_cast<size_t>(n_split) * (kHd + 2) : 0));
}

extern "C" int transoar_dense_attn_forward(const void* q, const void* k, const void* v, const unsigned* keybits, const int* bounds,
                                           void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Nq, long L,
                                           int C, int H, int O, int rows_per_organ, float scale, int n_split, void* hip_stream) {
  if (!q || !k || !v || !o || !lse || (keybits && !bounds)) return TRANSOAR_DENSEATTN_ERR_NULL;
  if (const int rc = check_dims(B, Nq, L, C, H, O, rows_per_organ, keybits != nullptr, n_split)) return rc;
  if (!(scale > 0.f)) return TRANSOAR_DENSEATTN_ERR_DIM;
  if (n_split > 1 && (!workspace || workspace_bytes < transoar_dense_attn_workspace_bytes(B, Nq, n_split)))
    return TRANSOAR_DENSEATTN_ERR_WORKSPACE;
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(o) || misaligned(keybits) || (n_split > 1 && misaligned(workspace)))
    return TRANSOAR_DENSEATTN_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int n_l = static_cast<int>(L), stride = (n_l + 31) / 32;
  const int rpo = keybits ? rows_per_organ : Nq;
  Workspace w{nullptr, nullptr, nullptr, nullptr};
  if (n_split > 1) w = carve(workspace, B, Nq, n_split);
  const dim3 grid(n_split, (Nq + kStage - 1) / kStage, B * kDH);
  hipLaunchKernelGGL(dense_attn_fwd, grid, dim3(256), 0, st, static_cast<const unsigned short*>(q), static_cast<const unsigned short*>(k),
                     static_cast<const unsigned short*>(v), keybits, keybits ? bounds : nullptr, static_cast<unsigned short*>(o), lse,
                     w.pacc, w.pm, w.pl, Nq, n_l, rpo, stride, scale * kLog2e, n_split);
  if (n_split > 1) {
    const long items = static_cast<long>(B) * kDH * Nq * 12;
    hipLaunchKernelGGL(dense_attn_fwd_combine, dim3(static_cast<unsigned>((items + 255) / 256)), dim3(256), 0, st, w.pacc, w.pm, w.pl,
                       static_cast<unsigned short*>(o), lse, Nq, n_split, items);
  }
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_dense_attn_backward(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                                            const float* lse, const unsigned* keybits, const int* bounds, void* dq, void* dk,
                                            void* dv, void* workspace, size_t workspace_bytes, int B, int Nq, long L, int C, int H,
                                            int O, int rows_per_organ, float scale, int n_split, void* hip_stream) {
  if (!q || !k || !v || !o || !d_o || !lse || !dq || !dk || !dv || !workspace || (keybits && !bounds)) return TRANSOAR_DENSEATTN_ERR_NULL;
  if (const int rc = check_dims(B, Nq, L, C, H, O, rows_per_organ, keybits != nullptr, n_split)) return rc;
  if (!(scale > 0.f)) return TRANSOAR_DENSEATTN_ERR_DIM;
  if (workspace_bytes < transoar_dense_attn_workspace_bytes(B, Nq, n_split)) return TRANSOAR_DENSEATTN_ERR_WORKSPACE;
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(o) || misaligned(d_o) || misaligned(dq) || misaligned(dk) ||
      misaligned(dv) || misaligned(keybits) || misaligned(workspace))
    return TRANSOAR_DENSEATTN_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int n_l = static_cast<int>(L), stride = (n_l + 31) / 32;
  const int rpo = keybits ? rows_per_organ : Nq, n_org = keybits ? O : 1;
  const int* bnd = keybits ? bounds : nullptr;
  const Workspace w = carve(workspace, B, Nq, n_split);
  const unsigned short *qs = static_cast<const unsigned short*>(q), *ks = static_cast<const unsigned short*>(k),
                       *vs = static_cast<const unsigned short*>(v), *ds = static_cast<const unsigned short*>(d_o);
  const long rows = static_cast<long>(B) * kDH * Nq;
  hipLaunchKernelGGL(dense_attn_delta, dim3(static_cast<unsigned>((rows + 255) / 256)), dim3(256), 0, st,
                     static_cast<const unsigned short*>(o), ds, w.delta, Nq, rows);
  const dim3 grid(n_split, (Nq + kStage - 1) / kStage, B * kDH);
  hipLaunchKernelGGL(dense_attn_bwd_q, grid, dim3(256), 0, st, qs, ks, vs, ds, lse, w.delta, keybits, bnd,
                     static_cast<unsigned short*>(dq), w.pacc, Nq, n_l, rpo, stride, scale, n_split);
  if (n_split > 1)
    hipLaunchKernelGGL(dense_attn_dq_combine, dim3(static_cast<unsigned>((rows * 12 + 255) / 256)), dim3(256), 0, st, w.pacc,
                       static_cast<unsigned short*>(dq), Nq, n_split, scale, rows * 12);
  hipLaunchKernelGGL(dense_attn_bwd_kv, dim3((n_l + kStage - 1) / kStage, B * kDH), dim3(256), 0, st, qs, ks, vs, ds, lse, w.delta,
                     keybits, bnd, static_cast<unsigned short*>(dk), static_cast<unsigned short*>(dv), Nq, n_l, n_org, rpo, stride,
                     scale);
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_denseattn_abi_version(void) { return 1; }
