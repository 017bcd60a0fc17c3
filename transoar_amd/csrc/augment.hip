// Batch augmentation for gfx950 (include/transoar_augment.h): range scaling, one trilinear resample through a per-sample affine
// map (nearest for the labels) and gain / offset, in one launch that writes both outputs.
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
// No LDS, no atomics, no dependence between lanes: the outputs are bitwise reproducible.
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
