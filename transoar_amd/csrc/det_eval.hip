// Detection records of a validation pass for gfx950 (include/transoar_deteval.h): the per-organ decode of
// transoar/inference.py and the IoU of transoar/utils/bboxes.py:150-186 for every (image, class) of a batch, appended to
// device buffers in ONE launch of ONE workgroup, with no atomics and no host synchronisation.
//
//   * Every thread reads the cursor first (a uniform load).  A batch that does not fit (cursor + n > capacity, or a cursor that
//     is not a row of the arrays at all) writes nothing but overflow = 1: the pair loop is skipped as a whole, so no address
//     past the arrays is formed.
//   * Wave w takes the pairs w, w + 4, ...; its lanes stride over the organ's qpo logits, keep (probability, index) of their
//     best and the wave reduces the pair with six xor shuffles: larger probability first, lower index among equals.  A NaN
//     probability enters as -1, below every number.  Lanes 0..5 copy the chosen box, lane 0 computes the IoU and stores the
//     scalars.
//   * After the barrier thread 0 advances the cursor and threads < n_losses add their loss in fp64: one thread per address,
//     launches of one stream are ordered, so the sums are plain read-modify-writes.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/transoar_deteval.h"

namespace {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;

template <typename T> __device__ __forceinline__ float load_f(const T* p, long i);
template <> __device__ __forceinline__ float load_f<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float load_f<unsigned short>(const unsigned short* p, long i) {      // bf16
  return __uint_as_float(static_cast<unsigned>(p[i]) << 16);
}
template <> __device__ __forceinline__ float load_f<__half>(const __half* p, long i) { return __half2float(p[i]); }

// iou_3d_np of one box pair, both cx cy cz w h d: fp32, numpy's order of operations, nothing contracted
__device__ __forceinline__ float iou_cxcyczwhd(const float* a, const float* b) {
#pragma clang fp contract(off)
  float a1[3], a2[3], b1[3], b2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a1[d] = a[d] - 0.5f * a[3 + d];
    a2[d] = a[d] + 0.5f * a[3 + d];
    b1[d] = b[d] - 0.5f * b[3 + d];
    b2[d] = b[d] + 0.5f * b[3 + d];
  }
  const float va = (a2[0] - a1[0]) * (a2[1] - a1[1]) * (a2[2] - a1[2]);
  const float vb = (b2[0] - b1[0]) * (b2[1] - b1[1]) * (b2[2] - b1[2]);
  float delta[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float lo = a1[d] > b1[d] ? a1[d] : b1[d];
    const float hi = a2[d] < b2[d] ? a2[d] : b2[d];
    const float e = hi - lo;
    delta[d] = e < 0.f ? 0.f : e;
  }
  const float inter = delta[0] * delta[1] * delta[2];
  const float uni = (va + vb) - inter;
  return inter / uni;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void det_eval_accumulate(const T* __restrict__ logits, const T* __restrict__ boxes,
                                                                const float* __restrict__ gt_boxes,
                                                                const unsigned char* __restrict__ gt_present,
                                                                const float* __restrict__ losses, int n_losses, int n, int k, int qpo,
                                                                int* __restrict__ state, int capacity, float* __restrict__ rec_score,
                                                                float* __restrict__ rec_iou, unsigned char* __restrict__ rec_has_gt,
                                                                int* __restrict__ rec_query, float* __restrict__ rec_box,
                                                                double* __restrict__ loss_sums) {
#pragma clang fp contract(off)
  const int cursor = state[0];
  const bool fits = cursor >= 0 && n <= capacity && cursor <= capacity - n;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (fits) {
    const int pairs = n * k;                                    // <= 65536
    for (int p = wave; p < pairs; p += kWaves) {
      const long first = static_cast<long>(p) * qpo;            // query (s, c * qpo) is row p * qpo
      float best = -2.f;
      int at = INT_MAX;
      for (int j = lane; j < qpo; j += kWave) {
        const float x = load_f<T>(logits, first + j);
        const float prob = 1.f / (1.f + expf(-x));
        const float key = prob != prob ? -1.f : prob;
        if (key > best) {                                       // j grows: the first of equals stays
          best = key;
          at = j;
        }
      }
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
        const float other = __shfl_xor(best, o, kWave);
        const int other_at = __shfl_xor(at, o, kWave);
        if (other > best || (other == best && other_at < at)) {
          best = other;
          at = other_at;
        }
      }
      // at is in 0..qpo-1 on every lane: lane 0 always holds j = 0 with a key of at least -1
      const long row = static_cast<long>(cursor) * k + p;       // (cursor + s) * k + c
      const long chosen = (first + at) * 6;
      if (lane < 6) rec_box[row * 6 + lane] = load_f<T>(boxes, chosen + lane);
      if (lane == 0) {
        const float x = load_f<T>(logits, first + at);
        rec_score[row] = 1.f / (1.f + expf(-x));
        rec_query[row] = at;
        const bool has = gt_present[p] != 0;
        float iou = -1.f;
        if (has) {
          float mine[6], truth[6];
#pragma unroll
          for (int d = 0; d < 6; ++d) {
            mine[d] = load_f<T>(boxes, chosen + d);
            truth[d] = gt_boxes[static_cast<long>(p) * 6 + d];
          }
          iou = iou_cxcyczwhd(mine, truth);
        }
        rec_iou[row] = iou;
        rec_has_gt[row] = has ? 1 : 0;
      }
    }
  }
  __syncthreads();                                              // every wave has read the cursor
  if (threadIdx.x == 0) {
    if (fits) state[0] = cursor + n;
    else state[1] = 1;
  }
  if (fits && losses != nullptr && static_cast<int>(threadIdx.x) < n_losses)
    loss_sums[threadIdx.x] = loss_sums[threadIdx.x] + static_cast<double>(losses[threadIdx.x]);
}

bool aligned(const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

}  // namespace

extern "C" int transoar_deteval_accumulate(const void* logits, const void* boxes, int dtype, const float* gt_boxes,
                                           const unsigned char* gt_present, const float* losses, int n_losses, int n, int k, int qpo,
                                           int* state, int capacity, float* rec_score, float* rec_iou, unsigned char* rec_has_gt,
                                           int* rec_query, float* rec_box, double* loss_sums, void* hip_stream) {
  if (!logits || !boxes || !gt_boxes || !gt_present || !state || !rec_score || !rec_iou || !rec_has_gt || !rec_query || !rec_box)
    return TRANSOAR_DETEVAL_ERR_NULL;
  if (n_losses < 0 || n_losses > TRANSOAR_DETEVAL_MAX_LOSSES) return TRANSOAR_DETEVAL_ERR_DIM;
  if (losses && n_losses > 0 && !loss_sums) return TRANSOAR_DETEVAL_ERR_NULL;
  if (k < 1 || k > TRANSOAR_DETEVAL_MAX_K || qpo < 1 || qpo > TRANSOAR_DETEVAL_MAX_QPO || n < 1 || n > TRANSOAR_DETEVAL_MAX_N ||
      capacity < 1 || capacity > TRANSOAR_DETEVAL_MAX_CAPACITY)
    return TRANSOAR_DETEVAL_ERR_DIM;
  if (dtype != TRANSOAR_DETEVAL_F32 && dtype != TRANSOAR_DETEVAL_BF16 && dtype != TRANSOAR_DETEVAL_F16) return TRANSOAR_DETEVAL_ERR_DTYPE;
  const size_t es = dtype == TRANSOAR_DETEVAL_F32 ? 4 : 2;
  if (!aligned(logits, es) || !aligned(boxes, es) || !aligned(gt_boxes, 4) || !aligned(losses, 4) || !aligned(state, 4) ||
      !aligned(rec_score, 4) || !aligned(rec_iou, 4) || !aligned(rec_query, 4) || !aligned(rec_box, 4) || !aligned(loss_sums, 8))
    return TRANSOAR_DETEVAL_ERR_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
#define TRANSOAR_DETEVAL_LAUNCH(T)                                                                                               \
  hipLaunchKernelGGL(det_eval_accumulate<T>, dim3(1), dim3(kThreads), 0, st, static_cast<const T*>(logits),                       \
                     static_cast<const T*>(boxes), gt_boxes, gt_present, losses, n_losses, n, k, qpo, state, capacity, rec_score, \
                     rec_iou, rec_has_gt, rec_query, rec_box, loss_sums)
  switch (dtype) {
    case TRANSOAR_DETEVAL_F32: TRANSOAR_DETEVAL_LAUNCH(float); break;
    case TRANSOAR_DETEVAL_BF16: TRANSOAR_DETEVAL_LAUNCH(unsigned short); break;
    default: TRANSOAR_DETEVAL_LAUNCH(__half); break;
  }
#undef TRANSOAR_DETEVAL_LAUNCH
  return static_cast<int>(hipGetLastError());
}

extern "C" int transoar_deteval_abi_version(void) { return 1; }
