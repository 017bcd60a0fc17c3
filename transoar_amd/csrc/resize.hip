// Case resize for gfx950 (include/transoar_resize.h): an adaptive-average ("area") resize of the image and torch's fp32 nearest
// rule for its label map, both through a per-sample crop window, in one launch that writes both outputs; and the foreground
// window of a label map in two launches.
//
//   * resize_area: grid (ceil(items / 256), n), items = dout * hout * ceil(wout / 4).  A lane owns four consecutive outputs
//     (d, h, w0 .. w0 + 3) of sample blockIdx.y.  The sample's window row (12 ints, wave-uniform: scalar loads) is clamped
//     first.  The bin edges floor(o E / R) are exact integer quotients -- 32-bit divisions when R * S < 2^32 on every axis (a
//     launch-uniform branch), 64-bit otherwise; the five edges of a lane's four W bins are computed once (the upper edge of bin
//     o is the quotient of o + 1, plus one where that division leaves a remainder).  The lane walks its D x H bin rows and, in
//     each row, the one contiguous span [lo(w0), hi(w0 + 3)) of source voxels: every voxel is loaded once and added to the bins
//     that contain it (one when downsampling, up to two neighbouring bins when upsampling), so per bin the sum runs D outermost,
//     W innermost, ascending.  Adjacent lanes' spans are adjacent in memory: a wave's direct loads cover one contiguous stretch
//     of a source row per (D, H) step.  The labels are read only at the picked points.
//   * kVec (wout % 4 == 0, outputs 16-byte aligned): the four fp32 outputs leave as one 16-byte store and the four labels as one
//     packed store.  Otherwise scalar stores, the row's tail masked.
//   * fg_scan: grid (B, n).  Workgroup (b, s) owns voxels [b * chunk, (b + 1) * chunk) of sample s, read 16 bytes per lane (a
//     scalar head up to the first 16-byte boundary and a scalar tail).  A lane keeps its minima / maxima in registers and folds
//     them into the workgroup's six LDS words with integer atomics once; the six words leave as one workspace row, written in
//     full.  fg_finalize: grid (n), reduces the B rows of its sample, applies the margins and writes the whole window row.
// No float atomics and no dependence between lanes in resize_area; integer minima / maxima in the window: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/transoar_resize.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;               // consecutive W outputs of a lane
constexpr long kMinChunk = 4096;          // voxels a workgroup of fg_scan takes at least
constexpr long kMaxChunk = 1L << 30;      // offsets inside a chunk are 32-bit
constexpr int kMaxRows = 1024;            // workgroups of fg_scan over the whole batch, unless kMaxChunk asks for more
constexpr int kUnroll = 4;                // 16-byte loads a lane of fg_scan has in flight

template <typename T> struct alignas(sizeof(T) * kPerLane < 16 ? sizeof(T) * kPerLane : 16) Pack {
  T e[kPerLane];
};

struct Geometry {
  int S[3];              // source extents
  int R[3];              // the resized grid
  int O[3];              // the part of it that is written
  unsigned groups;       // lanes per output row: ceil(O[2] / 4)
  unsigned items;        // lanes per sample
  long vin, vout;        // voxels per input / output sample
  int narrow;            // R * S < 2^32 on every axis: 32-bit quotients
  int scale;             // range scaling on
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floor(o * e / r) and whether the division leaves a remainder; o <= r, so the quotient is at most e
__device__ __forceinline__ int edge(int o, int e, int r, bool narrow, bool& rem) {
  const unsigned long a = static_cast<unsigned long>(o) * static_cast<unsigned long>(e);
  if (narrow) {
    const unsigned q = static_cast<unsigned>(a) / static_cast<unsigned>(r);
    rem = q * static_cast<unsigned>(r) != static_cast<unsigned>(a);
    return static_cast<int>(q);
  }
  const unsigned long q = a / static_cast<unsigned long>(r);
  rem = q * static_cast<unsigned long>(r) != a;
  return static_cast<int>(q);
}

// torch's nearest source index, computed in fp32
__device__ __forceinline__ int nearest(int o, int e, int r) {
  const float scale = static_cast<float>(e) / static_cast<float>(r);          // IEEE division (hipcc's default for fp32)
  const int i = static_cast<int>(floorf(static_cast<float>(o) * scale));
  return i < e - 1 ? i : e - 1;
}

template <typename TI> __device__ __forceinline__ float value(TI x, bool scale, float a_min, float range) {
  const float f = static_cast<float>(x);
  if (!scale) return f;
  const float v = (f - a_min) / range;
  return fminf(fmaxf(v, 0.f), 1.f);
}

template <typename TI, typename T, bool kLabels, bool kVec>
__global__ __launch_bounds__(kThreads) void resize_area(const TI* __restrict__ image, const T* __restrict__ labels,
                                                        const int* __restrict__ window, float* __restrict__ image_out,
                                                        T* __restrict__ labels_out, Geometry g, float a_min, float range) {
  const unsigned item = blockIdx.x * static_cast<unsigned>(kThreads) + threadIdx.x;
  if (item >= g.items) return;
  const unsigned n = blockIdx.y;
  // the sample's window, clamped: start in [0, S - 1], extent in [1, S - start], crop in [0, R - out]
  int st[3], ex[3], cr[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int s = 0, e = g.S[a], c = 0;
    if (window) {
      const int* row = window + static_cast<long>(n) * TRANSOAR_RSZ_WINDOW;
      s = row[a], e = row[3 + a], c = row[6 + a];
    }
    st[a] = clampi(s, 0, g.S[a] - 1);
    ex[a] = clampi(e, 1, g.S[a] - st[a]);
    cr[a] = clampi(c, 0, g.R[a] - g.O[a]);
  }
  const bool narrow = g.narrow != 0, scale = g.scale != 0;
  const unsigned row = item / g.groups;
  const int w0 = static_cast<int>(item - row * g.groups) * kPerLane;
  const int d = static_cast<int>(row / static_cast<unsigned>(g.O[1]));
  const int h = static_cast<int>(row - static_cast<unsigned>(d) * static_cast<unsigned>(g.O[1]));
  const int od = cr[0] + d, oh = cr[1] + h, ow = cr[2] + w0;         // indices of the resized grid; od < R[0], oh < R[1]

  bool rem;
  const int dlo = edge(od, ex[0], g.R[0], narrow, rem);
  int dhi = edge(od + 1, ex[0], g.R[0], narrow, rem);
  dhi += rem ? 1 : 0;
  const int hlo = edge(oh, ex[1], g.R[1], narrow, rem);
  int hhi = edge(oh + 1, ex[1], g.R[1], narrow, rem);
  hhi += rem ? 1 : 0;
  int lo[kPerLane], hi[kPerLane];
  {
    int q[kPerLane + 1];
    bool r[kPerLane + 1];
#pragma unroll
    for (int k = 0; k <= kPerLane; ++k) {
      const int o = ow + k < g.R[2] ? ow + k : g.R[2];               // an output past the row's end: an empty bin at E
      q[k] = edge(o, ex[2], g.R[2], narrow, r[k]);
    }
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      lo[j] = q[j];
      hi[j] = w0 + j < g.O[2] ? q[j + 1] + (r[j + 1] ? 1 : 0) : q[j];
    }
  }
  int span_hi = lo[0];                                               // hi[] is not monotonic where a masked bin is empty
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) span_hi = hi[j] > span_hi ? hi[j] : span_hi;

  const long origin = static_cast<long>(n) * g.vin + (static_cast<long>(st[0]) * g.S[1] + st[1]) * g.S[2] + st[2];
  const TI* src = image + origin;
  float acc[kPerLane] = {0.f, 0.f, 0.f, 0.f};
  for (int zd = dlo; zd < dhi; ++zd) {
    for (int zh = hlo; zh < hhi; ++zh) {
      const TI* line = src + (static_cast<long>(zd) * g.S[1] + zh) * g.S[2];
      // one loop over the span, every voxel selected into its bins.  Both neighbours of this form measured SLOWER (DESIGN
      // 12.11): two rows x eight predicated loads issued together (+12-17 %), and one plain loop per bin without selects (+16-25 %)
      for (int zw = lo[0]; zw < span_hi; ++zw) {
        const float v = value<TI>(line[zw], scale, a_min, range);
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) acc[j] += (zw >= lo[j] && zw < hi[j]) ? v : 0.f;
      }
    }
  }
  Pack<float> out;
  const long plane = static_cast<long>(dhi - dlo) * (hhi - hlo);     // < 2^48
#pragma unroll
  for (int j = 0; j < kPerLane; ++j)                                 // an empty bin: an output past the row's end, not stored
    out.e[j] = hi[j] > lo[j] ? acc[j] / static_cast<float>(plane * (hi[j] - lo[j])) : 0.f;

  Pack<T> lab;
  if (kLabels) {
    const T* lsrc = labels + origin;
    const long base = (static_cast<long>(nearest(od, ex[0], g.R[0])) * g.S[1] + nearest(oh, ex[1], g.R[1])) * g.S[2];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int o = ow + j < g.R[2] ? ow + j : g.R[2] - 1;
      lab.e[j] = lsrc[base + nearest(o, ex[2], g.R[2])];
    }
  }

  const long o = static_cast<long>(n) * g.vout + static_cast<long>(row) * g.O[2] + w0;
  if (kVec) {
    *reinterpret_cast<Pack<float>*>(image_out + o) = out;
    if (kLabels) *reinterpret_cast<Pack<T>*>(labels_out + o) = lab;
  } else {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      if (w0 + j < g.O[2]) {
        image_out[o + j] = out.e[j];
        if (kLabels) labels_out[o + j] = lab.e[j];
      }
    }
  }
}

// ---- the foreground window -------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ bool selected(T l, long mask) {
  if (mask < 0) return l > static_cast<T>(0);
  return l >= static_cast<T>(1) && l <= static_cast<T>(62) && ((mask >> static_cast<int>(l)) & 1L) != 0;
}

// position of the voxel `o` voxels after the chunk's first, which sits at (x0, y0, z0)
__device__ __forceinline__ void locate(unsigned o, int x0, int y0, int z0, unsigned sy, unsigned sz, int& x, int& y, int& z) {
  const unsigned t = static_cast<unsigned>(z0) + o;
  const unsigned rows = t / sz;
  z = static_cast<int>(t - rows * sz);
  const unsigned u = static_cast<unsigned>(y0) + rows;
  const unsigned planes = u / sy;
  y = static_cast<int>(u - planes * sy);
  x = x0 + static_cast<int>(planes);
}

struct Extremes {
  int mn[3], mx[3];
  __device__ __forceinline__ void take(int x, int y, int z) {
    mn[0] = x < mn[0] ? x : mn[0], mn[1] = y < mn[1] ? y : mn[1], mn[2] = z < mn[2] ? z : mn[2];
    mx[0] = x > mx[0] ? x : mx[0], mx[1] = y > mx[1] ? y : mx[1], mx[2] = z > mx[2] ? z : mx[2];
  }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void fg_scan(const T* __restrict__ labels, long V, int sy, int sz, long mask, long chunk,
                                                    int* __restrict__ slab) {
  constexpr int E = 16 / sizeof(T);
  __shared__ int tab[6];
  if (threadIdx.x < 6) tab[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : -1;
  __syncthreads();
  Extremes m;
#pragma unroll
  for (int a = 0; a < 3; ++a) m.mn[a] = INT_MAX, m.mx[a] = -1;
  const long v0 = static_cast<long>(blockIdx.x) * chunk;
  const long v1 = v0 + chunk < V ? v0 + chunk : V;
  if (v0 < v1) {
    const unsigned cnt = static_cast<unsigned>(v1 - v0);
    const long plane = static_cast<long>(sy) * sz;
    const int x0 = static_cast<int>(v0 / plane);
    const long rem = v0 - x0 * plane;
    const int y0 = static_cast<int>(rem / sz), z0 = static_cast<int>(rem - static_cast<long>(y0) * sz);
    const T* p = labels + static_cast<long>(blockIdx.y) * V + v0;
    unsigned head = static_cast<unsigned>(((16u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T));
    if (head > cnt) head = cnt;
    const unsigned nvec = (cnt - head) / E;
    const unsigned tail = head + nvec * E;
    // the scalar ends: fewer than E voxels each
    {
      unsigned o = cnt;
      if (threadIdx.x < head) o = threadIdx.x;
      else if (threadIdx.x >= 32 && tail + (threadIdx.x - 32) < cnt) o = tail + (threadIdx.x - 32);
      if (o < cnt && selected<T>(p[o], mask)) {
        int x, y, z;
        locate(o, x0, y0, z0, sy, sz, x, y, z);
        m.take(x, y, z);
      }
    }
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    for (unsigned base = 0; base < nvec; base += kThreads * kUnroll) {
      union {
        uint4 q;
        T e[E];
      } u[kUnroll];
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) {
        const unsigned i = base + j * kThreads + threadIdx.x;
        u[j].q = i < nvec ? pv[i] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int j = 0; j < kUnroll; ++j) {
        if ((u[j].q.x | u[j].q.y | u[j].q.z | u[j].q.w) == 0u) continue;          // background only (or past the end)
        const unsigned i = base + j * kThreads + threadIdx.x;
        int x, y, z;
        locate(head + i * E, x0, y0, z0, sy, sz, x, y, z);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (selected<T>(u[j].e[e], mask)) m.take(x, y, z);
          if (++z == sz) {
            z = 0;
            if (++y == sy) {
              y = 0;
              ++x;
            }
          }
        }
      }
    }
  }
  if (m.mx[0] >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(tab + a, m.mn[a]);
      atomicMax(tab + 3 + a, m.mx[a]);
    }
  }
  __syncthreads();
  int* row = slab + (static_cast<long>(blockIdx.y) * gridDim.x + blockIdx.x) * 6;
  if (threadIdx.x < 6) row[threadIdx.x] = tab[threadIdx.x];
}

struct Margins {
  int S[3], m[3];
};

__global__ __launch_bounds__(kThreads) void fg_finalize(const int* __restrict__ slab, int B, Margins g, int* __restrict__ window) {
  __shared__ int tab[6];
  if (threadIdx.x < 6) tab[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : -1;
  __syncthreads();
  constexpr int groups = kThreads / 6;
  const int grp = threadIdx.x / 6, item = threadIdx.x - grp * 6;
  if (grp < groups) {
    const bool is_lo = item < 3;
    const int* rows = slab + static_cast<long>(blockIdx.x) * B * 6 + item;
    int acc = is_lo ? INT_MAX : -1;
    for (int r = grp; r < B; r += groups) {
      const int v = rows[static_cast<long>(r) * 6];
      acc = is_lo ? (v < acc ? v : acc) : (v > acc ? v : acc);
    }
    if (is_lo) atomicMin(tab + item, acc);
    else atomicMax(tab + item, acc);
  }
  __syncthreads();
  if (threadIdx.x < TRANSOAR_RSZ_WINDOW) {
    const bool found = tab[3] >= 0;
    const int t = threadIdx.x, a = t % 3;
    int start = 0, end = g.S[a];
    if (found) {
      start = tab[a] - g.m[a];
      start = start < 0 ? 0 : start;
      const long e = static_cast<long>(tab[3 + a]) + 1 + g.m[a];
      end = e < g.S[a] ? static_cast<int>(e) : g.S[a];
    }
    int v = 0;
    if (t < 3) v = start;
    else if (t < 6) v = end - start;
    else if (t == 9) v = found ? 1 : 0;
    window[static_cast<long>(blockIdx.x) * TRANSOAR_RSZ_WINDOW + t] = v;
  }
}

int elem_size(int dt) {
  switch (dt) {
    case TRANSOAR_RSZ_U8: return 1;
    case TRANSOAR_RSZ_I16: return 2;
    case TRANSOAR_RSZ_I32: return 4;
    case TRANSOAR_RSZ_I64: return 8;
    default: return 0;
  }
}

bool extent_ok(int s) { return s >= 1 && s <= TRANSOAR_RSZ_MAX_EXTENT; }

// voxels of a sample, or 0 where it has 2^40 or more
long sample_voxels(int d, int h, int w) {
  const long plane = static_cast<long>(d) * h;           // < 2^48
  if (plane > (1L << 40) / w) return 0;
  const long v = plane * w;
  return v < (1L << 40) ? v : 0;
}

bool fg_dims_ok(int n, long V) { return n >= 1 && n <= 65535 && V >= 1 && V < (1L << 40); }

// workgroups per sample: at least kMinChunk voxels each, about kMaxRows over the batch, no chunk above kMaxChunk
long blocks_per_sample(int n, long V) {
  long b = (V + kMinChunk - 1) / kMinChunk;
  const long cap = kMaxRows / n > 1 ? kMaxRows / n : 1;
  if (b > cap) b = cap;
  const long need = (V + kMaxChunk - 1) / kMaxChunk;
  return b > need ? b : need;
}

template <typename TI, typename T, bool kLabels>
void launch(bool vec, dim3 grid, hipStream_t st, const void* image, const void* labels, const int* window, float* image_out,
            void* labels_out, const Geometry& g, float a_min, float range) {
  if (vec)
    hipLaunchKernelGGL((resize_area<TI, T, kLabels, true>), grid, dim3(kThreads), 0, st, static_cast<const TI*>(image),
                       static_cast<const T*>(labels), window, image_out, static_cast<T*>(labels_out), g, a_min, range);
  else
    hipLaunchKernelGGL((resize_area<TI, T, kLabels, false>), grid, dim3(kThreads), 0, st, static_cast<const TI*>(image),
                       static_cast<const T*>(labels), window, image_out, static_cast<T*>(labels_out), g, a_min, range);
}

template <typename TI>
void launch_image(int label_dtype, bool vec, dim3 grid, hipStream_t st, const void* image, const void* labels, const int* window,
                  float* image_out, void* labels_out, const Geometry& g, float a_min, float range) {
  if (!labels) {
    launch<TI, unsigned char, false>(vec, grid, st, image, nullptr, window, image_out, nullptr, g, a_min, range);
    return;
  }
  switch (label_dtype) {
    case TRANSOAR_RSZ_U8: launch<TI, unsigned char, true>(vec, grid, st, image, labels, window, image_out, labels_out, g, a_min, range); break;
    case TRANSOAR_RSZ_I16: launch<TI, short, true>(vec, grid, st, image, labels, window, image_out, labels_out, g, a_min, range); break;
    case TRANSOAR_RSZ_I32: launch<TI, int, true>(vec, grid, st, image, labels, window, image_out, labels_out, g, a_min, range); break;
    default: launch<TI, long long, true>(vec, grid, st, image, labels, window, image_out, labels_out, g, a_min, range); break;
  }
}

}  // namespace

extern "C" int transoar_resize_forward(const void* image, int image_dtype, const void* labels, int label_dtype, int n, int di, int hi,
                                       int wi, int rd, int rh, int rw, int dout, int hout, int wout, const int* window,
                                       int scale_range, float a_min, float a_max, float* image_out, void* labels_out,
                                       void* hip_stream) {
  if (!image || !image_out || (labels == nullptr) != (labels_out == nullptr)) return TRANSOAR_RSZ_ERR_NULL;
  if (n < 1 || n > 65535 || !extent_ok(di) || !extent_ok(hi) || !extent_ok(wi) || !extent_ok(rd) || !extent_ok(rh) || !extent_ok(rw))
    return TRANSOAR_RSZ_ERR_DIM;
  if (dout < 1 || hout < 1 || wout < 1 || dout > rd || hout > rh || wout > rw) return TRANSOAR_RSZ_ERR_DIM;
  if (scale_range && (!isfinite(a_min) || !isfinite(a_max) || !(a_max > a_min) || !isfinite(a_max - a_min))) return TRANSOAR_RSZ_ERR_DIM;
  Geometry g;
  g.S[0] = di, g.S[1] = hi, g.S[2] = wi;
  g.R[0] = rd, g.R[1] = rh, g.R[2] = rw;
  g.O[0] = dout, g.O[1] = hout, g.O[2] = wout;
  g.vin = sample_voxels(di, hi, wi);
  if (!g.vin) return TRANSOAR_RSZ_ERR_DIM;
  const long rows = static_cast<long>(dout) * hout;         // <= 2^48
  if (rows >= (1L << 33) || rows * wout >= (1L << 33)) return TRANSOAR_RSZ_ERR_DIM;          // rows * wout < 2^57
  g.vout = rows * wout;
  g.groups = static_cast<unsigned>((wout + kPerLane - 1) / kPerLane);
  const long items = static_cast<long>(dout) * hout * g.groups;          // <= vout < 2^33
  if (items > 0x7fffff00L) return TRANSOAR_RSZ_ERR_DIM;                  // item indices are 32-bit, the block that holds the last one included
  g.items = static_cast<unsigned>(items);
  g.narrow = 1;
  for (int a = 0; a < 3; ++a)
    if (static_cast<long>(g.R[a]) * g.S[a] >= (1L << 32)) g.narrow = 0;
  g.scale = scale_range ? 1 : 0;
  const int is = image_dtype == TRANSOAR_RSZ_F32 ? 4 : (image_dtype == TRANSOAR_RSZ_I16 ? 2 : 0);
  if (!is) return TRANSOAR_RSZ_ERR_DTYPE;
  int es = 1;
  if (labels) {
    es = elem_size(label_dtype);
    if (!es) return TRANSOAR_RSZ_ERR_DTYPE;
  }
  if (reinterpret_cast<uintptr_t>(image) % is || reinterpret_cast<uintptr_t>(window) % sizeof(int) ||
      reinterpret_cast<uintptr_t>(image_out) % sizeof(float) || reinterpret_cast<uintptr_t>(labels) % es ||
      reinterpret_cast<uintptr_t>(labels_out) % es)
    return TRANSOAR_RSZ_ERR_ALIGN;
  const uintptr_t pack = es * kPerLane < 16 ? es * kPerLane : 16;
  const bool vec = wout % kPerLane == 0 && reinterpret_cast<uintptr_t>(image_out) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(labels_out) % pack == 0;
  const dim3 grid(static_cast<unsigned>((items + kThreads - 1) / kThreads), static_cast<unsigned>(n));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const float lo = scale_range ? a_min : 0.f, range = scale_range ? a_max - a_min : 1.f;
  if (image_dtype == TRANSOAR_RSZ_F32)
    launch_image<float>(label_dtype, vec, grid, st, image, labels, window, image_out, labels_out, g, lo, range);
  else
    launch_image<short>(label_dtype, vec, grid, st, image, labels, window, image_out, labels_out, g, lo, range);
  return static_cast<int>(hipGetLastError());
}

extern "C" size_t transoar_foreground_window_workspace_bytes(int n, long voxels_per_sample) {
  if (!fg_dims_ok(n, voxels_per_sample)) return 0;
  return static_cast<size_t>(n) * blocks_per_sample(n, voxels_per_sample) * 6 * sizeof(int);
}

extern "C" int transoar_foreground_window(const void* labels, int label_dtype, int n, int sd, int sh, int sw, long class_mask,
                                          int margin_d, int margin_h, int margin_w, int* window, void* workspace,
                                          size_t workspace_bytes, void* hip_stream) {
  if (!labels || !window || !workspace) return TRANSOAR_RSZ_ERR_NULL;
  if (!extent_ok(sd) || !extent_ok(sh) || !extent_ok(sw)) return TRANSOAR_RSZ_ERR_DIM;
  if (margin_d < 0 || margin_h < 0 || margin_w < 0 || margin_d > TRANSOAR_RSZ_MAX_EXTENT || margin_h > TRANSOAR_RSZ_MAX_EXTENT ||
      margin_w > TRANSOAR_RSZ_MAX_EXTENT)
    return TRANSOAR_RSZ_ERR_DIM;
  const long V = sample_voxels(sd, sh, sw);
  if (!V || !fg_dims_ok(n, V)) return TRANSOAR_RSZ_ERR_DIM;
  const int es = elem_size(label_dtype);
  if (!es) return TRANSOAR_RSZ_ERR_DTYPE;
  if (workspace_bytes < transoar_foreground_window_workspace_bytes(n, V)) return TRANSOAR_RSZ_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(labels) % es || reinterpret_cast<uintptr_t>(workspace) % sizeof(int) ||
      reinterpret_cast<uintptr_t>(window) % sizeof(int))
    return TRANSOAR_RSZ_ERR_ALIGN;
  const long B = blocks_per_sample(n, V);
  const long chunk = (V + B - 1) / B;
  const dim3 grid(static_cast<unsigned>(B), static_cast<unsigned>(n));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int* slab = static_cast<int*>(workspace);
#define TRANSOAR_RSZ_LAUNCH(T) \
  hipLaunchKernelGGL(fg_scan<T>, grid, dim3(kThreads), 0, st, static_cast<const T*>(labels), V, sh, sw, class_mask, chunk, slab)
  switch (label_dtype) {
    case TRANSOAR_RSZ_U8: TRANSOAR_RSZ_LAUNCH(unsigned char); break;
    case TRANSOAR_RSZ_I16: TRANSOAR_RSZ_LAUNCH(short); break;
    case TRANSOAR_RSZ_I32: TRANSOAR_RSZ_LAUNCH(int); break;
    default: TRANSOAR_RSZ_LAUNCH(long long); break;
  }
#undef TRANSOAR_RSZ_LAUNCH
  Margins m;
  m.S[0] = sd, m.S[1] = sh, m.S[2] = sw;
  m.m[0] = margin_d, m.m[1] = margin_h, m.m[2] = margin_w;
  hipLaunchKernelGGL(fg_finalize, dim3(static_cast<unsigned>(n)), dim3(kThreads), 0, st, slab, static_cast<int>(B), m, window);
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_resize_abi_version(void) { return 1; }
