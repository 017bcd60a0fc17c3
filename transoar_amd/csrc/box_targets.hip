// Detection targets from label volumes for gfx950 (include/transoar_boxtargets.h): segmentation2bbox of
// transoar/utils/bboxes.py:45-96 as two launches, with no float atomics and no host synchronisation.
//
//   * box_scan: grid (B, n).  Workgroup (b, s) owns voxels [b * chunk, (b + 1) * chunk) of sample s -- a contiguous run of memory,
//     read 16 bytes per lane (a scalar head up to the first 16-byte boundary and a scalar tail: a sample need not start on
//     one).  A 16-byte group that is all background costs one OR of four words.  Otherwise the lane finds the (x, y, z) of its
//     first voxel with two 32-bit divisions, walks its voxels carrying z -> y -> x (a group may span several rows) and collapses
//     runs of equal labels within a row; a run updates the workgroup's k x 6 LDS table of minima / maxima with integer LDS
//     atomics, each only where a plain read says it would change the entry (the entries are monotonic, so a stale read can only
//     cost an unneeded atomic).  The table leaves as one row of the workspace, written in full.
//   * box_finalize: one workgroup.  Per sample the B rows are reduced by 1024 / (6 k) thread groups (coalesced rows), combined in
//     LDS, and thread c applies the reference's rule to class c + 1; the present classes are counted in an LDS integer.
// Minima, maxima and an integer count are order-independent, so the outputs are bitwise reproducible, and every workspace word
// box_finalize reads was written by box_scan of the same call.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/transoar_boxtargets.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFinalThreads = 1024;
constexpr long kMinChunk = 4096;          // voxels a workgroup takes at least (one 16-byte round of uint8 labels)
constexpr long kMaxChunk = 1L << 30;      // offsets inside a chunk are 32-bit
constexpr int kMaxRows = 1024;            // workgroups (= workspace rows) over the whole batch, unless kMaxChunk asks for more
constexpr int kUnroll = 4;                // 16-byte loads a lane has in flight
constexpr int kFinalLoads = 16;           // workspace rows a thread of box_finalize has in flight

__device__ __forceinline__ void table_init(int* tab, int items, int threads) {
  for (int i = threadIdx.x; i < items; i += threads) tab[i] = (i % 6) < 3 ? INT_MAX : -1;
}

// voxels (x, y, zlo..zhi) carry class c (1-based)
__device__ __forceinline__ void table_update(int* tab, int c, int x, int y, int zlo, int zhi) {
  int* t = tab + (c - 1) * 6;
  const volatile int* r = t;
  if (x < r[0]) atomicMin(t + 0, x);
  if (y < r[1]) atomicMin(t + 1, y);
  if (zlo < r[2]) atomicMin(t + 2, zlo);
  if (x > r[3]) atomicMax(t + 3, x);
  if (y > r[4]) atomicMax(t + 4, y);
  if (zhi > r[5]) atomicMax(t + 5, zhi);
}

template <typename T> __device__ __forceinline__ int class_of(T l, int k) {
  return (l >= static_cast<T>(1) && l <= static_cast<T>(k)) ? static_cast<int>(l) : 0;      // 0: not a class of the targets
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

template <typename T>
__global__ __launch_bounds__(kThreads) void box_scan(const T* __restrict__ labels, long V, int sy, int sz, int k, long chunk,
                                                     int* __restrict__ slab) {
  constexpr int E = 16 / sizeof(T);
  __shared__ int tab[TRANSOAR_BOX_MAX_K * 6];
  const int items = k * 6;
  table_init(tab, items, kThreads);
  __syncthreads();
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
      if (o < cnt) {
        const int c = class_of<T>(p[o], k);
        if (c) {
          int x, y, z;
          locate(o, x0, y0, z0, sy, sz, x, y, z);
          table_update(tab, c, x, y, z, z);
        }
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
        int cur = 0, zs = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int c = class_of<T>(u[j].e[e], k);
          if (c != cur) {
            if (cur) table_update(tab, cur, x, y, zs, z - 1);
            cur = c;
            zs = z;
          }
          if (++z == sz) {                   // the row ends: so does the run
            if (cur) table_update(tab, cur, x, y, zs, z - 1);
            cur = 0;
            z = 0;
            if (++y == sy) {
              y = 0;
              ++x;
            }
          }
        }
        if (cur) table_update(tab, cur, x, y, zs, z - 1);
      }
    }
  }
  __syncthreads();
  int* row = slab + (static_cast<long>(blockIdx.y) * gridDim.x + blockIdx.x) * items;
  for (int i = threadIdx.x; i < items; i += kThreads) row[i] = tab[i];
}

__global__ __launch_bounds__(kFinalThreads) void box_finalize(const int* __restrict__ slab, int n, int B, int k, int sx, int sy, int sz,
                                                              int padding, int min_extent, float* __restrict__ boxes,
                                                              unsigned char* __restrict__ present, float* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ int tab[TRANSOAR_BOX_MAX_K * 6];
  __shared__ int total;
  const int items = k * 6;
  const int groups = kFinalThreads / items;          // >= 2 (items <= 384)
  const int g = threadIdx.x / items, item = threadIdx.x - g * items;
  const bool is_lo = (item % 6) < 3;
  if (threadIdx.x == 0) total = 0;
  for (int s = 0; s < n; ++s) {
    table_init(tab, items, kFinalThreads);
    __syncthreads();
    if (g < groups) {
      const int* rows = slab + static_cast<long>(s) * B * items + item;
      int acc = is_lo ? INT_MAX : -1;
      int r = g;
      for (; r + (kFinalLoads - 1) * groups < B; r += kFinalLoads * groups) {      // independent loads, issued together
        int v[kFinalLoads];
#pragma unroll
        for (int u = 0; u < kFinalLoads; ++u) v[u] = rows[static_cast<long>(r + u * groups) * items];
#pragma unroll
        for (int u = 0; u < kFinalLoads; ++u) acc = is_lo ? (v[u] < acc ? v[u] : acc) : (v[u] > acc ? v[u] : acc);
      }
      for (; r < B; r += groups) {
        const int v = rows[static_cast<long>(r) * items];
        acc = is_lo ? (v < acc ? v : acc) : (v > acc ? v : acc);
      }
      if (is_lo) atomicMin(tab + item, acc);
      else atomicMax(tab + item, acc);
    }
    __syncthreads();
    if (threadIdx.x < k) {
      const int* t = tab + threadIdx.x * 6;
      const int size[3] = {sx, sy, sz};
      bool here = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) here = here && t[3 + a] >= t[a] && t[3 + a] - t[a] >= min_extent;
      float out[6];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float fs = static_cast<float>(size[a]);
        float lo = static_cast<float>(t[a]) - static_cast<float>(padding);
        lo = lo < 0.f ? 0.f : lo;
        float hi = static_cast<float>(t[3 + a]) + static_cast<float>(padding);
        hi = hi > fs ? fs : hi;
        lo = lo / fs;
        hi = hi / fs;
        out[a] = (hi + lo) / 2.f;
        out[3 + a] = hi - lo;
      }
      float* bx = boxes + (static_cast<long>(s) * k + threadIdx.x) * 6;
#pragma unroll
      for (int a = 0; a < 6; ++a) bx[a] = here ? out[a] : 0.f;
      present[static_cast<long>(s) * k + threadIdx.x] = here ? 1 : 0;
      if (here) atomicAdd(&total, 1);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] = static_cast<float>(total);
    counts[1] = static_cast<float>(total);
  }
}

int elem_size(int dt) {
  switch (dt) {
    case TRANSOAR_BOX_U8: return 1;
    case TRANSOAR_BOX_I16: return 2;
    case TRANSOAR_BOX_I32: return 4;
    case TRANSOAR_BOX_I64: return 8;
    default: return 0;
  }
}

bool dims_ok(int n, long V, int k) { return n >= 1 && n <= 65535 && V >= 1 && V < (1L << 40) && k >= 1 && k <= TRANSOAR_BOX_MAX_K; }

// workgroups per sample: at least kMinChunk voxels each, about kMaxRows over the batch, no chunk above kMaxChunk
long blocks_per_sample(int n, long V) {
  long b = (V + kMinChunk - 1) / kMinChunk;
  const long cap = kMaxRows / n > 1 ? kMaxRows / n : 1;
  if (b > cap) b = cap;
  const long need = (V + kMaxChunk - 1) / kMaxChunk;
  return b > need ? b : need;
}

}  // namespace

extern "C" size_t transoar_box_targets_workspace_bytes(int n, long voxels_per_sample, int k) {
  if (!dims_ok(n, voxels_per_sample, k)) return 0;
  return static_cast<size_t>(n) * blocks_per_sample(n, voxels_per_sample) * k * 6 * sizeof(int);
}

extern "C" int transoar_box_targets_forward(const void* labels, int label_dtype, int n, int sx, int sy, int sz, int k, int padding,
                                            int min_extent, float* boxes, unsigned char* present, float* counts, void* workspace,
                                            size_t workspace_bytes, void* hip_stream) {
  if (!labels || !boxes || !present || !counts || !workspace) return TRANSOAR_BOX_ERR_NULL;
  if (sx < 1 || sy < 1 || sz < 1 || padding < 0 || min_extent < 0) return TRANSOAR_BOX_ERR_DIM;
  const long plane = static_cast<long>(sx) * sy;           // < 2^62
  if (plane > (1L << 40) / sz) return TRANSOAR_BOX_ERR_DIM;
  const long V = plane * sz;
  if (!dims_ok(n, V, k)) return TRANSOAR_BOX_ERR_DIM;
  const int es = elem_size(label_dtype);
  if (!es || workspace_bytes < transoar_box_targets_workspace_bytes(n, V, k)) return TRANSOAR_BOX_ERR_DTYPE;
  if (reinterpret_cast<uintptr_t>(labels) % es || reinterpret_cast<uintptr_t>(workspace) % sizeof(int)) return TRANSOAR_BOX_ERR_ALIGN;
  const long B = blocks_per_sample(n, V);
  const long chunk = (V + B - 1) / B;
  const dim3 grid(static_cast<unsigned>(B), static_cast<unsigned>(n));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int* slab = static_cast<int*>(workspace);
#define TRANSOAR_BOX_LAUNCH(T) \
  hipLaunchKernelGGL(box_scan<T>, grid, dim3(kThreads), 0, st, static_cast<const T*>(labels), V, sy, sz, k, chunk, slab)
  switch (label_dtype) {
    case TRANSOAR_BOX_U8: TRANSOAR_BOX_LAUNCH(unsigned char); break;
    case TRANSOAR_BOX_I16: TRANSOAR_BOX_LAUNCH(short); break;
    case TRANSOAR_BOX_I32: TRANSOAR_BOX_LAUNCH(int); break;
    default: TRANSOAR_BOX_LAUNCH(long long); break;
  }
#undef TRANSOAR_BOX_LAUNCH
  hipLaunchKernelGGL(box_finalize, dim3(1), dim3(kFinalThreads), 0, st, slab, n, static_cast<int>(B), k, sx, sy, sz, padding,
                     min_extent, boxes, present, counts);
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_boxtargets_abi_version(void) { return 1; }
