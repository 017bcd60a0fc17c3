// Batch augmentation for gfx950 (include/transoar_augment.h): range scaling, one trilinear resample through a per-sample affine
// map (nearest for the labels) and gain / offset, in one launch that writes both outputs; and, below it, the intensity tail
// (noise, Gaussian smoothing, gain / offset, gamma contrast) as its own launch sequence.
//
//   * augment_resample: grid (ceil(items / 256), n), items = dout * hout * ceil(wout / 4).  A lane owns four consecutive outputs
//     (d, h, w0 .. w0 + 3) of sample blockIdx.y; consecutive lanes walk a W row, so at the small angles and zooms of the shipped
//     chain neighbouring lanes read neighbouring addresses and the eight corner loads are served by L1 / L2.  The sample's table
//     row is wave-uniform (scalar loads).  The source coordinate is  M (d, h, w) + t  in fp64 FMAs on the fp32 table (nine per
//     output: nothing next to the loads), so that the interpolation weights carry one fp32 rounding and not the rounding of a
//     coordinate of magnitude 2^5..2^8 -- in fp32 that alone costs 1.5e-4 relative on small outputs.  Whether the coordinate is
//     usable (finite, within +-2^24) is decided on the float, and only a usable one is converted to an integer.  Every corner load
//     is predicated on the corner lying inside the volume AND carrying a non-zero weight: an integer-exact map (identity, flips,
//     shifts, the validation crop) therefore loads one corner per output, not eight, with no second kernel.
//   * kVec (wout % 4 == 0, outputs 16-byte aligned): the four fp32 outputs leave as one 16-byte store and the four labels as one
//     packed store (4 / 8 / 16 / 2 x 16 bytes).  Otherwise scalar stores, the row's tail masked.
// The resample uses no LDS, no atomics and has no dependence between lanes: its outputs are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/transoar_augment.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;                        // consecutive W outputs of a lane
constexpr double kMaxCoord = 16777216.0;           // TRANSOAR_AUG_MAX_EXTENT

template <typename T> struct alignas(sizeof(T) * kPerLane < 16 ? sizeof(T) * kPerLane : 16) Pack {
  T e[kPerLane];
};

struct Geometry {
  int di, hi, wi;        // input extents
  int ho, wo;            // output extents (dout is implied by items)
  unsigned groups;       // lanes per output row: ceil(wo / 4)
  unsigned items;        // lanes per sample
  long vin, vout;        // voxels per input / output sample
};

__device__ __forceinline__ float scaled(float x, float a_min, float range) {
  const float v = (x - a_min) / range;             // IEEE division (hipcc's default for fp32)
  return fminf(fmaxf(v, 0.f), 1.f);
}

// One axis of the trilinear stencil: i0 = floor(s) and the weights of i0 / i0 + 1; in[] says which of the two lies in [0, size).
struct Axis {
  int i0;
  float w[2];
  bool in[2];
};

__device__ __forceinline__ Axis axis_of(double s, bool usable, int size) {
  const double f = usable ? floor(s) : 0.0;        // the conversion below only ever sees an integer within +-2^24
  Axis a;
  a.i0 = static_cast<int>(f);
  a.w[1] = usable ? static_cast<float>(s - f) : 0.f;
  a.w[0] = usable ? 1.f - a.w[1] : 0.f;
  a.in[0] = usable && a.i0 >= 0 && a.i0 < size;
  a.in[1] = usable && a.i0 + 1 >= 0 && a.i0 + 1 < size;
  return a;
}

template <typename T, bool kLabels, bool kVec>
__global__ __launch_bounds__(kThreads) void augment_resample(const float* __restrict__ image, const T* __restrict__ labels,
                                                             const float* __restrict__ params, float* __restrict__ image_out,
                                                             T* __restrict__ labels_out, Geometry g, float a_min, float range) {
  const unsigned item = blockIdx.x * static_cast<unsigned>(kThreads) + threadIdx.x;
  if (item >= g.items) return;
  const unsigned n = blockIdx.y;
  const float* p = params + static_cast<long>(n) * TRANSOAR_AUG_PARAMS;
  const unsigned row = item / g.groups;
  const int w0 = static_cast<int>(item - row * g.groups) * kPerLane;
  const int d = static_cast<int>(row / static_cast<unsigned>(g.ho));
  const int h = static_cast<int>(row - static_cast<unsigned>(d) * static_cast<unsigned>(g.ho));
  const double fd = static_cast<double>(d), fh = static_cast<double>(h);
  // the part of M o + t that the row shares
  const double bd = fma(static_cast<double>(p[1]), fh, fma(static_cast<double>(p[0]), fd, static_cast<double>(p[3])));
  const double bh = fma(static_cast<double>(p[5]), fh, fma(static_cast<double>(p[4]), fd, static_cast<double>(p[7])));
  const double bw = fma(static_cast<double>(p[9]), fh, fma(static_cast<double>(p[8]), fd, static_cast<double>(p[11])));
  const double cd = p[2], ch = p[6], cw = p[10];
  const float gain = p[12], offset = p[13];
  const float* src = image + static_cast<long>(n) * g.vin;
  const T* lsrc = kLabels ? labels + static_cast<long>(n) * g.vin : nullptr;

  Pack<float> out;
  Pack<T> lab;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const double fw = static_cast<double>(w0 + j);
    const double sd = fma(cd, fw, bd), sh = fma(ch, fw, bh), sw = fma(cw, fw, bw);
    // not finite, or beyond +-2^24: outside (a NaN fails every comparison)
    const bool usable = w0 + j < g.wo && fabs(sd) <= kMaxCoord && fabs(sh) <= kMaxCoord && fabs(sw) <= kMaxCoord;
    const Axis ad = axis_of(sd, usable, g.di), ah = axis_of(sh, usable, g.hi), aw = axis_of(sw, usable, g.wi);
    float x[8], wgt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {                  // all eight loads are issued before the first is used
      const int kd = c >> 2, kh = (c >> 1) & 1, kw = c & 1;
      wgt[c] = (ad.w[kd] * ah.w[kh]) * aw.w[kw];
      x[c] = 0.f;
      if (ad.in[kd] && ah.in[kh] && aw.in[kw] && wgt[c] != 0.f)
        x[c] = src[(static_cast<long>(ad.i0 + kd) * g.hi + (ah.i0 + kh)) * g.wi + (aw.i0 + kw)];
      else
        wgt[c] = 0.f;
    }
    if (kLabels) {
      const double rd = usable ? floor(sd + 0.5) : -1.0, rh = usable ? floor(sh + 0.5) : -1.0, rw = usable ? floor(sw + 0.5) : -1.0;
      const int id = static_cast<int>(rd), ih = static_cast<int>(rh), iw = static_cast<int>(rw);
      T l = static_cast<T>(0);
      if (id >= 0 && id < g.di && ih >= 0 && ih < g.hi && iw >= 0 && iw < g.wi)
        l = lsrc[(static_cast<long>(id) * g.hi + ih) * g.wi + iw];
      lab.e[j] = l;
    }
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc += wgt[c] != 0.f ? wgt[c] * scaled(x[c], a_min, range) : 0.f;
    out.e[j] = __fadd_rn(__fmul_rn(acc, gain), offset);         // two roundings
  }

  const long o = static_cast<long>(n) * g.vout + static_cast<long>(row) * g.wo + w0;
  if (kVec) {
    *reinterpret_cast<Pack<float>*>(image_out + o) = out;
    if (kLabels) *reinterpret_cast<Pack<T>*>(labels_out + o) = lab;
  } else {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      if (w0 + j < g.wo) {
        image_out[o + j] = out.e[j];
        if (kLabels) labels_out[o + j] = lab.e[j];
      }
    }
  }
}

int elem_size(int dt) {
  switch (dt) {
    case TRANSOAR_AUG_U8: return 1;
    case TRANSOAR_AUG_I16: return 2;
    case TRANSOAR_AUG_I32: return 4;
    case TRANSOAR_AUG_I64: return 8;
    default: return 0;
  }
}

template <typename T, bool kLabels>
void launch(bool vec, dim3 grid, hipStream_t st, const float* image, const void* labels, const float* params, float* image_out,
            void* labels_out, const Geometry& g, float a_min, float range) {
  if (vec)
    hipLaunchKernelGGL((augment_resample<T, kLabels, true>), grid, dim3(kThreads), 0, st, image, static_cast<const T*>(labels), params,
                       image_out, static_cast<T*>(labels_out), g, a_min, range);
  else
    hipLaunchKernelGGL((augment_resample<T, kLabels, false>), grid, dim3(kThreads), 0, st, image, static_cast<const T*>(labels), params,
                       image_out, static_cast<T*>(labels_out), g, a_min, range);
}

}  // namespace

extern "C" int transoar_augment_forward(const float* image, const void* labels, int label_dtype, int n, int di, int hi, int wi,
                                        int dout, int hout, int wout, const float* params, float a_min, float a_max,
                                        float* image_out, void* labels_out, void* hip_stream) {
  if (!image || !params || !image_out || (labels == nullptr) != (labels_out == nullptr)) return TRANSOAR_AUG_ERR_NULL;
  if (n < 1 || n > 65535 || di < 1 || hi < 1 || wi < 1 || dout < 1 || hout < 1 || wout < 1) return TRANSOAR_AUG_ERR_DIM;
  if (di > TRANSOAR_AUG_MAX_EXTENT || hi > TRANSOAR_AUG_MAX_EXTENT || wi > TRANSOAR_AUG_MAX_EXTENT) return TRANSOAR_AUG_ERR_DIM;
  if (dout > di || hout > hi || wout > wi) return TRANSOAR_AUG_ERR_DIM;
  if (!isfinite(a_min) || !isfinite(a_max) || !(a_max > a_min) || !isfinite(a_max - a_min)) return TRANSOAR_AUG_ERR_DIM;
  const long plane = static_cast<long>(di) * hi;            // < 2^48
  if (plane > (1L << 40) / wi) return TRANSOAR_AUG_ERR_DIM;
  Geometry g;
  g.di = di, g.hi = hi, g.wi = wi, g.ho = hout, g.wo = wout;
  g.vin = plane * wi;
  g.vout = static_cast<long>(dout) * hout * wout;           // <= vin < 2^41
  if (g.vin >= (1L << 40) || g.vout >= (1L << 33)) return TRANSOAR_AUG_ERR_DIM;
  g.groups = static_cast<unsigned>((wout + kPerLane - 1) / kPerLane);
  const long items = static_cast<long>(dout) * hout * g.groups;          // <= vout < 2^33
  if (items > 0x7fffff00L) return TRANSOAR_AUG_ERR_DIM;                  // item indices are 32-bit, the block that holds the last one included
  g.items = static_cast<unsigned>(items);
  int es = 1;
  if (labels) {
    es = elem_size(label_dtype);
    if (!es) return TRANSOAR_AUG_ERR_DTYPE;
  }
  if (reinterpret_cast<uintptr_t>(image) % sizeof(float) || reinterpret_cast<uintptr_t>(params) % sizeof(float) ||
      reinterpret_cast<uintptr_t>(image_out) % sizeof(float) || reinterpret_cast<uintptr_t>(labels) % es ||
      reinterpret_cast<uintptr_t>(labels_out) % es)
    return TRANSOAR_AUG_ERR_ALIGN;
  const uintptr_t pack = es * kPerLane < 16 ? es * kPerLane : 16;
  const bool vec = wout % kPerLane == 0 && reinterpret_cast<uintptr_t>(image_out) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(labels_out) % pack == 0;
  const dim3 grid(static_cast<unsigned>((items + kThreads - 1) / kThreads), static_cast<unsigned>(n));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const float range = a_max - a_min;
  if (!labels) {
    launch<unsigned char, false>(vec, grid, st, image, nullptr, params, image_out, nullptr, g, a_min, range);
  } else {
    switch (label_dtype) {
      case TRANSOAR_AUG_U8: launch<unsigned char, true>(vec, grid, st, image, labels, params, image_out, labels_out, g, a_min, range); break;
      case TRANSOAR_AUG_I16: launch<short, true>(vec, grid, st, image, labels, params, image_out, labels_out, g, a_min, range); break;
      case TRANSOAR_AUG_I32: launch<int, true>(vec, grid, st, image, labels, params, image_out, labels_out, g, a_min, range); break;
      default: launch<long long, true>(vec, grid, st, image, labels, params, image_out, labels_out, g, a_min, range); break;
    }
  }
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_augment_abi_version(void) { return 1; }

// ---- the intensity tail (transoar_augment_intensity): noise -> smooth -> gain / offset -> gamma contrast ---------------------------
//
//   * intensity_prepare, grid n: reads a table row ONCE, validates it and leaves in the workspace what the other kernels take as
//     block-uniform scalars: the three radii (0 when the sample does not smooth), the effective flags, the scalars, the three
//     normalised weight vectors (fp64 erf, rounded once; padded with zeros to 40 entries, tap x at [19 + x], so that a window
//     that is wider than the stencil reads zeros and never leaves the array) and the min / max cells at their identities.  No
//     later kernel looks at the table: whatever it holds, radii are in 0..16 and every index is formed from them.
//   * intensity_plane (steps has the smooth bit): image -> scratch, noise + W filter + H filter of a 32 x 64 tile of one D plane.
//     The patch (32 + 2 r_h) x (64 + 2 R), R = r_w rounded up to 4, is staged in LDS with the noise already added (a voxel's
//     noise depends on (key, linear index) only, so a halo voxel gets the value its own tile gives it); outside voxels are 0.
//     A lane owns four consecutive W outputs and reads the patch as 16-byte chunks: the W filter walks R / 2 + 1 chunks and
//     multiplies each of their 16 (input, output) pairs with the weight of their distance (zero beyond r_w), the H filter one
//     chunk per tap.  Row strides of 128 (patch) and 64 (intermediate) floats keep the 16-lane groups of ds_read_b128 on
//     distinct banks.  48 KiB of LDS: three blocks per CU.
//   * intensity_finish<true>: scratch -> image_out, D filter (2 r_d + 1 coalesced 16-byte loads per lane, served by L2 / MALL:
//     neighbouring planes are read by neighbouring blocks), gain / offset, and the block's min / max into one of the sample's 32
//     workspace cells with one integer atomic each on the order-preserving encoding (the contrast kernel folds the 32 cells).  intensity_finish<false> is the whole tail without smoothing:
//     image -> image_out with the noise added in registers.
//   * intensity_contrast (steps has the contrast bit): the power law in place.
// A radius of 0 copies, no noise adds nothing and gain 1 / offset 0 is skipped: such a sample comes out bit-identical.
namespace {

constexpr int kTailWords = 12;
constexpr int kMaxRadius = 16;
constexpr int kWPad = 40;                          // padded weights of an axis
constexpr int kWCentre = 19;                       // tap x at [kWCentre + x]; |x| <= kMaxRadius + 3
constexpr int kCells = 32;                         // min / max cells of a sample, 64 bytes apart; a block adds to cell blockIdx.x % 32
constexpr int kCellWords = 16;
enum { WS_RD = 0, WS_RH, WS_RW, WS_FLAGS, WS_MEAN, WS_STD, WS_GAIN, WS_OFFSET, WS_GAMMA, WS_K0, WS_K1, WS_AFFINE,
       WS_WEIGHTS = 16,                            // D at 16, H at 56, W at 96
       WS_CELLS = 144 };                           // cell c: min at [144 + 16 c], max at [145 + 16 c]
constexpr int kWsWords = WS_CELLS + kCells * kCellWords;        // 656 words per sample
constexpr int kTH = 32, kTW = 64;                  // outputs of a block of intensity_plane
constexpr int kPRows = kTH + 2 * kMaxRadius;       // 64
constexpr int kPStride = 128, kMStride = 64;       // floats per patch / intermediate row

struct TailGeom {
  int d, h, w;
  int vec;               // w % 4 == 0 and every pointer 16-byte aligned: 16-byte loads and stores
  unsigned groups;       // lanes per row: ceil(w / 4)
  unsigned items;        // lanes per sample
  unsigned tiles_h, tiles_w;
  long vol;
};

__device__ __forceinline__ unsigned ordered(float x) {          // unsigned order == float order
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float unordered(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__global__ __launch_bounds__(128) void intensity_prepare(const unsigned* __restrict__ table, unsigned steps, unsigned* __restrict__ ws) {
  __shared__ double raw[3 * kWPad];
  const unsigned* row = table + static_cast<long>(blockIdx.x) * kTailWords;
  unsigned* out = ws + static_cast<long>(blockIdx.x) * kWsWords;
  const int t = threadIdx.x;
  unsigned flags = row[0] & steps & 7u;
  const float sig[3] = {__uint_as_float(row[3]), __uint_as_float(row[4]), __uint_as_float(row[5])};
  bool smooth = (flags & 2u) != 0;
  int tail[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    smooth = smooth && sig[a] > 0.f && sig[a] <= 4.f;            // false for a NaN
    tail[a] = 0;
  }
  if (smooth) {
#pragma unroll
    for (int a = 0; a < 3; ++a) tail[a] = min(static_cast<int>(fmaxf(4.f * sig[a], 0.5f) + 0.5f), kMaxRadius);
  }
  const int a = t / kWPad, x = t - a * kWPad - kWCentre;
  if (t < 3 * kWPad) {
    double w = x == 0 ? 1.0 : 0.0;
    if (smooth) {
      const float sg = a == 0 ? sig[0] : a == 1 ? sig[1] : sig[2];
      const int r = a == 0 ? tail[0] : a == 1 ? tail[1] : tail[2];
      const double tt = 0.70710678 / static_cast<double>(sg);
      w = 0.0;
      if (x >= -r && x <= r) w = fmax(0.5 * (erf(tt * (x + 0.5)) - erf(tt * (x - 0.5))), 0.0);
    }
    raw[t] = w;
  }
  __syncthreads();
  if (t < 3 * kWPad) {
    double sum = 0.0;
    for (int i = 0; i < kWPad; ++i) sum += raw[a * kWPad + i];
    out[WS_WEIGHTS + t] = __float_as_uint(static_cast<float>(raw[t] / sum));
  }
  if (t == 0) {
    const float mean = __uint_as_float(row[1]), sd = __uint_as_float(row[2]), gamma = __uint_as_float(row[8]);
    float gain = __uint_as_float(row[6]), offset = __uint_as_float(row[7]);
    if (!isfinite(mean) || !isfinite(sd)) flags &= ~1u;
    if (!smooth) flags &= ~2u;
    if (!isfinite(gamma) || !(gamma > 0.f)) flags &= ~4u;
    if (!isfinite(gain)) gain = 1.f;
    if (!isfinite(offset)) offset = 0.f;
    out[WS_RD] = tail[0], out[WS_RH] = tail[1], out[WS_RW] = tail[2];
    out[WS_FLAGS] = flags;
    out[WS_MEAN] = __float_as_uint(mean), out[WS_STD] = __float_as_uint(sd);
    out[WS_GAIN] = __float_as_uint(gain), out[WS_OFFSET] = __float_as_uint(offset), out[WS_GAMMA] = __float_as_uint(gamma);
    out[WS_K0] = row[9], out[WS_K1] = row[10];
    out[WS_AFFINE] = (gain != 1.f || offset != 0.f) ? 1u : 0u;
  }
  if (t < kCells) out[WS_CELLS + kCellWords * t] = ordered(INFINITY), out[WS_CELLS + kCellWords * t + 1] = ordered(-INFINITY);
}

// Philox4x32-10 on the counter (j lo, j hi, 0, 0) and four normals from its four words (Box-Muller, accurate logf / sincospif).
__device__ __forceinline__ void normals(long j, unsigned k0, unsigned k1, float z[4]) {
  unsigned c0 = static_cast<unsigned>(j), c1 = static_cast<unsigned>(static_cast<unsigned long>(j) >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  const unsigned r[4] = {c0, c1, c2, c3};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (static_cast<float>(r[2 * p] >> 9) + 0.5f) * 0x1p-23f;      // exact
    const float u2 = static_cast<float>(r[2 * p + 1] >> 9) * 0x1p-23f;          // exact
    const float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(2.f * u2, &s, &c);
    z[2 * p] = rad * c, z[2 * p + 1] = rad * s;
  }
}

// the normals of the voxels i0 .. i0 + 3 of a sample (i0 >= -3; a voxel below 0 gets a value nobody uses)
__device__ __forceinline__ void noise4(long i0, unsigned k0, unsigned k1, float z[4]) {
  float a[4];
  normals(i0 >> 2, k0, k1, a);
  const int s = static_cast<int>(i0 & 3);
  if (s == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = a[e];
    return;
  }
  float b[4];
  normals((i0 >> 2) + 1, k0, k1, b);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = s + e;                           // 1 .. 6
    z[e] = i == 1 ? a[1] : i == 2 ? a[2] : i == 3 ? a[3] : i == 4 ? b[0] : i == 5 ? b[1] : b[2];
  }
}

struct alignas(16) F4 {
  float e[4];
};

// four consecutive floats of a row from p + w0, those at w0 + e >= w (and below 0) left 0
__device__ __forceinline__ F4 load4(const float* p, int w0, int w, bool vec) {
  F4 v = {{0.f, 0.f, 0.f, 0.f}};
  if (vec) {
    v = *reinterpret_cast<const F4*>(p + w0);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (w0 + e >= 0 && w0 + e < w) v.e[e] = p[w0 + e];
  }
  return v;
}

__device__ __forceinline__ void store4(float* p, int w0, int w, bool vec, const F4& v) {
  if (vec) {
    *reinterpret_cast<F4*>(p + w0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (w0 + e < w) p[w0 + e] = v.e[e];
  }
}

__global__ __launch_bounds__(256) void intensity_plane(const float* __restrict__ image, float* __restrict__ scratch,
                                                       const unsigned* __restrict__ ws, TailGeom g) {
  __shared__ F4 patch[kPRows * kPStride / 4];      // 32 KiB
  __shared__ F4 mid[kPRows * kMStride / 4];        // 16 KiB
  const unsigned n = blockIdx.y;
  const unsigned* p = ws + static_cast<long>(n) * kWsWords;
  const int rh = static_cast<int>(p[WS_RH]), rw = static_cast<int>(p[WS_RW]);      // 0 .. 16, written by intensity_prepare
  const int R = (rw + 3) & ~3;
  const bool noise = (p[WS_FLAGS] & 1u) != 0;
  const float mean = __uint_as_float(p[WS_MEAN]), sd = __uint_as_float(p[WS_STD]);
  const unsigned k0 = p[WS_K0], k1 = p[WS_K1];
  const float* wt_h = reinterpret_cast<const float*>(p) + WS_WEIGHTS + kWPad + kWCentre;
  const float* wt_w = reinterpret_cast<const float*>(p) + WS_WEIGHTS + 2 * kWPad + kWCentre;
  unsigned b = blockIdx.x;
  const int tw = static_cast<int>(b % g.tiles_w);
  b /= g.tiles_w;
  const int th = static_cast<int>(b % g.tiles_h);
  const int d = static_cast<int>(b / g.tiles_h);
  const int h0 = th * kTH, w0 = tw * kTW;
  const int prow = kTH + 2 * rh, pgroups = (kTW + 2 * R) / 4;                    // <= 64, <= 24
  const long plane = static_cast<long>(d) * g.h * g.w;
  const float* src = image + static_cast<long>(n) * g.vol;
  const bool vec = g.vec != 0;
  const int tid = threadIdx.x;

  for (int it = tid; it < prow * pgroups; it += 256) {
    const int pr = it / pgroups, pg = it - pr * pgroups;
    const int hh = h0 - rh + pr, ww = w0 - R + 4 * pg;
    F4 v = {{0.f, 0.f, 0.f, 0.f}};
    if (hh >= 0 && hh < g.h && ww < g.w && ww + 3 >= 0) {
      const long row = plane + static_cast<long>(hh) * g.w;
      v = load4(src + row, ww, g.w, vec);          // vec: ww is a multiple of 4 in [0, w), the whole group is inside
      if (noise) {
        float z[4];
        noise4(row + ww, k0, k1, z);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ww + e >= 0 && ww + e < g.w) v.e[e] = v.e[e] + fmaf(sd, z[e], mean);     // one form in both kernels: the same bits
      }
    }
    patch[pr * (kPStride / 4) + pg] = v;
  }
  __syncthreads();

  for (int it = tid; it < prow * (kTW / 4); it += 256) {                       // the W filter: patch -> mid
    const int pr = it >> 4, gq = it & 15;
    F4 acc = patch[pr * (kPStride / 4) + gq];
    if (rw != 0) {
      acc = F4{{0.f, 0.f, 0.f, 0.f}};
      for (int k = 0; k <= R / 2; ++k) {           // chunk k holds the patch columns 4 (gq + k) + e; output j sits at R + 4 gq + j
        const F4 c = patch[pr * (kPStride / 4) + gq + k];
        const float* wk = wt_w + (4 * k - R);      // tap x = 4 k + e - R - j in [-R - 3, R + 3]: inside the padded array
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc.e[j] = fmaf(c.e[e], wk[e - j], acc.e[j]);
      }
    }
    mid[pr * (kMStride / 4) + gq] = acc;
  }
  __syncthreads();

  float* dst = scratch + static_cast<long>(n) * g.vol;
  for (int it = tid; it < kTH * (kTW / 4); it += 256) {                        // the H filter: mid -> scratch
    const int r = it >> 4, gq = it & 15;
    const int hh = h0 + r, ww = w0 + 4 * gq;
    if (hh >= g.h || ww >= g.w) continue;
    F4 acc = mid[(r + rh) * (kMStride / 4) + gq];
    if (rh != 0) {
      acc = F4{{0.f, 0.f, 0.f, 0.f}};
      for (int x = -rh; x <= rh; ++x) {
        const F4 c = mid[(r + rh + x) * (kMStride / 4) + gq];
        const float wx = wt_h[x];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc.e[j] = fmaf(c.e[j], wx, acc.e[j]);
      }
    }
    store4(dst + plane + static_cast<long>(hh) * g.w, ww, g.w, vec, acc);
  }
}

// kSmooth: in = scratch, the D filter.  Otherwise in = image (which may be image_out), the noise.  Then gain / offset, min / max.
template <bool kSmooth>
__global__ __launch_bounds__(256) void intensity_finish(const float* in, float* out, const unsigned* __restrict__ ws, unsigned* cells,
                                                        TailGeom g, int minmax) {
  __shared__ float part[2][4];
  const unsigned n = blockIdx.y;
  const unsigned* p = ws + static_cast<long>(n) * kWsWords;
  const unsigned item = blockIdx.x * 256u + threadIdx.x;
  const bool vec = g.vec != 0;
  float lo = INFINITY, hi = -INFINITY;
  if (item < g.items) {
    const unsigned row = item / g.groups;
    const int w0 = static_cast<int>(item - row * g.groups) * 4;
    const long base = static_cast<long>(n) * g.vol + static_cast<long>(row) * g.w;
    F4 v;
    if (kSmooth) {
      const int rd = static_cast<int>(p[WS_RD]);   // 0 .. 16
      const int d = static_cast<int>(row / static_cast<unsigned>(g.h));
      const long step = static_cast<long>(g.h) * g.w;
      v = load4(in + base, w0, g.w, vec);
      if (rd != 0) {
        const float* wt = reinterpret_cast<const float*>(p) + WS_WEIGHTS + kWCentre;
        v = F4{{0.f, 0.f, 0.f, 0.f}};
        for (int x = -rd; x <= rd; ++x) {
          if (d + x < 0 || d + x >= g.d) continue;
          const F4 c = load4(in + base + x * step, w0, g.w, vec);
          const float wx = wt[x];
#pragma unroll
          for (int j = 0; j < 4; ++j) v.e[j] = fmaf(c.e[j], wx, v.e[j]);
        }
      }
    } else {
      v = load4(in + base, w0, g.w, vec);
      if (p[WS_FLAGS] & 1u) {
        const float mean = __uint_as_float(p[WS_MEAN]), sd = __uint_as_float(p[WS_STD]);
        float z[4];
        noise4(static_cast<long>(row) * g.w + w0, p[WS_K0], p[WS_K1], z);
#pragma unroll
        for (int e = 0; e < 4; ++e) v.e[e] = v.e[e] + fmaf(sd, z[e], mean);     // one form in both kernels: the same bits
      }
    }
    if (p[WS_AFFINE]) {
      const float gain = __uint_as_float(p[WS_GAIN]), offset = __uint_as_float(p[WS_OFFSET]);
#pragma unroll
      for (int e = 0; e < 4; ++e) v.e[e] = __fadd_rn(__fmul_rn(v.e[e], gain), offset);          // two roundings
    }
    store4(out + base, w0, g.w, vec, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (w0 + e < g.w) lo = fminf(lo, v.e[e]), hi = fmaxf(hi, v.e[e]);
  }
  if (!minmax) return;                             // uniform
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = lo, part[1][threadIdx.x >> 6] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fminf(fminf(part[0][0], part[0][1]), fminf(part[0][2], part[0][3]));
    hi = fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]));
    // 32 cells per sample: thousands of blocks on one address serialise at the memory side (measured: 250 us per batch)
    unsigned* cell = cells + static_cast<long>(n) * kWsWords + WS_CELLS + kCellWords * (blockIdx.x % kCells);
    atomicMin(cell, ordered(lo));
    atomicMax(cell + 1, ordered(hi));
  }
}

__global__ __launch_bounds__(256) void intensity_contrast(float* image, const unsigned* __restrict__ ws, TailGeom g) {
  const unsigned n = blockIdx.y;
  const unsigned* p = ws + static_cast<long>(n) * kWsWords;
  const unsigned item = blockIdx.x * 256u + threadIdx.x;
  if (!(p[WS_FLAGS] & 4u)) return;                 // block-uniform
  __shared__ float ends[2];
  if (threadIdx.x < 64) {                          // the finishing step of the reduction: the sample's 32 cells
    const unsigned c = threadIdx.x % kCells;
    float lo = unordered(p[WS_CELLS + kCellWords * c]), hi = unordered(p[WS_CELLS + kCellWords * c + 1]);
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, off, 64));
      hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if (threadIdx.x == 0) ends[0] = lo, ends[1] = hi;
  }
  __syncthreads();
  if (item >= g.items) return;
  const float mn = ends[0], mx = ends[1], gamma = __uint_as_float(p[WS_GAMMA]);
  const float range = mx - mn, den = range + 1e-7f;
  const unsigned row = item / g.groups;
  const int w0 = static_cast<int>(item - row * g.groups) * 4;
  float* q = image + static_cast<long>(n) * g.vol + static_cast<long>(row) * g.w;
  const bool vec = g.vec != 0;
  F4 v = load4(q, w0, g.w, vec);
#pragma unroll
  for (int e = 0; e < 4; ++e) v.e[e] = __fadd_rn(__fmul_rn(powf(__fdiv_rn(v.e[e] - mn, den), gamma), range), mn);
  store4(q, w0, g.w, vec, v);
}

}  // namespace

extern "C" long transoar_augment_intensity_workspace_bytes(int n) {
  return n < 1 ? 0L : static_cast<long>(n) * kWsWords * static_cast<long>(sizeof(unsigned));
}

extern "C" int transoar_augment_intensity(const float* image, float* image_out, float* scratch, int n, int d, int h, int w,
                                          const void* table, int steps, void* workspace, void* hip_stream) {
  steps &= TRANSOAR_AUG_NOISE | TRANSOAR_AUG_SMOOTH | TRANSOAR_AUG_CONTRAST;
  const bool smooth = (steps & TRANSOAR_AUG_SMOOTH) != 0;
  if (!image || !image_out || !table || !workspace || (smooth && !scratch)) return TRANSOAR_AUG_ERR_NULL;
  if (n < 1 || n > 65535 || d < 1 || h < 1 || w < 1) return TRANSOAR_AUG_ERR_DIM;
  if (d > TRANSOAR_AUG_MAX_EXTENT || h > TRANSOAR_AUG_MAX_EXTENT || w > TRANSOAR_AUG_MAX_EXTENT) return TRANSOAR_AUG_ERR_DIM;
  TailGeom g;
  g.d = d, g.h = h, g.w = w;
  g.groups = static_cast<unsigned>((w + 3) / 4);
  const long rows = static_cast<long>(d) * h;                  // < 2^48
  if (rows > 0x7fffff00L / g.groups) return TRANSOAR_AUG_ERR_DIM;             // lane indices are 32-bit
  g.items = static_cast<unsigned>(rows * g.groups);
  g.vol = rows * w;
  g.tiles_h = static_cast<unsigned>((h + kTH - 1) / kTH), g.tiles_w = static_cast<unsigned>((w + kTW - 1) / kTW);
  const long tiles = static_cast<long>(g.tiles_h) * g.tiles_w * d;
  if (tiles > 0x7fffffffL) return TRANSOAR_AUG_ERR_DIM;
  const uintptr_t all = reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(image_out) |
                        reinterpret_cast<uintptr_t>(smooth ? scratch : nullptr);
  if (all % sizeof(float) || reinterpret_cast<uintptr_t>(table) % sizeof(unsigned) ||
      reinterpret_cast<uintptr_t>(workspace) % sizeof(unsigned))
    return TRANSOAR_AUG_ERR_ALIGN;
  g.vec = (w % 4 == 0 && all % 16 == 0) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const unsigned* tab = static_cast<const unsigned*>(table);
  unsigned* ws = static_cast<unsigned*>(workspace);
  const dim3 lanes((g.items + 255u) / 256u, static_cast<unsigned>(n));
  const int minmax = (steps & TRANSOAR_AUG_CONTRAST) ? 1 : 0;
  hipLaunchKernelGGL(intensity_prepare, dim3(static_cast<unsigned>(n)), dim3(128), 0, st, tab, static_cast<unsigned>(steps), ws);
  if (smooth) {
    hipLaunchKernelGGL(intensity_plane, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n)), dim3(256), 0, st, image, scratch,
                       ws, g);
    hipLaunchKernelGGL((intensity_finish<true>), lanes, dim3(256), 0, st, scratch, image_out, ws, ws, g, minmax);
  } else {
    hipLaunchKernelGGL((intensity_finish<false>), lanes, dim3(256), 0, st, image, image_out, ws, ws, g, minmax);
  }
  if (minmax) hipLaunchKernelGGL(intensity_contrast, lanes, dim3(256), 0, st, image_out, ws, g);
  return static_cast<int>(hipGetLastError());
}
