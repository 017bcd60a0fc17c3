/*
 * transoar_segproxy.h -- C ABI of the segmentation proxy loss for MI355X (gfx950): the 1x1x1 segmentation head on the
 * full-resolution FPN level P0 and the softmax cross-entropy + batch soft-Dice losses on its logits.
 *
 * Reference semantics: transoar/models/transoarnet.py:38-42,121,138 (the head: Conv3d(start_channels, K, kernel 1), K = 2
 * under fg_bg, else num_organs + 1) and transoar/models/criterion.py:77-90,127-197 (loss_segmentation: labels mapped to
 * (label > 0) under fg_bg, F.cross_entropy = mean over every voxel of -log softmax[label], SoftDiceLoss with batch_dice=True,
 * do_bg=False: dc_k = (2 tp_k + smooth_nom) / (2 tp_k + fp_k + fn_k + smooth_denom) summed over batch and space,
 * segdice = 1 - mean_{k >= 1} dc_k).
 *
 * Shapes: N samples, S = D * H * W voxels per sample, C input channels of the head (1 <= C <= 64), K classes
 * (head: 1 <= K <= 32, losses: 2 <= K <= 32).  A feature / logit map is (N, C or K, D, H, W) in one of two layouts:
 * TRANSOAR_SEG_NCDHW (contiguous) or TRANSOAR_SEG_NDHWC (channels-last: the channels of a voxel are adjacent).  Labels are
 * N * S contiguous integers ((N, 1, D, H, W) or (N, D, H, W)).  A label outside [0, K) (after the fg_bg mapping) is a caller
 * error, as in the reference; the kernels clamp it into [0, K - 1] so that no value reads or writes outside a buffer.
 *
 * All pointers are device pointers; asynchronous on `hip_stream`; capturable (no host synchronisation, no host read of a
 * device value; the upstream gradients of the losses are read on the device).  Every reduction over voxels is deterministic:
 * a fixed number of workgroups for a given shape, per-workgroup fp32 partial slabs in `workspace`, summed in a fixed order by a
 * second launch.  Returns 0, a hipError_t (> 0), or a negative TRANSOAR_SEG_ERR_* code (checked on the host, nothing printed).
 */
#ifndef TRANSOAR_SEGPROXY_H
#define TRANSOAR_SEGPROXY_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TRANSOAR_SEG_MAX_C 64
#define TRANSOAR_SEG_MAX_K 32
#define TRANSOAR_SEG_ERR_NULL (-1)
#define TRANSOAR_SEG_ERR_DIM (-2)
#define TRANSOAR_SEG_ERR_DTYPE (-3)
#define TRANSOAR_SEG_ERR_LAYOUT (-4)

/* storage types of maps (fp32 accumulation either way) */
#define TRANSOAR_SEG_F32 0
#define TRANSOAR_SEG_BF16 2
/* label types */
#define TRANSOAR_SEG_U8 16
#define TRANSOAR_SEG_I16 17
#define TRANSOAR_SEG_I32 18
#define TRANSOAR_SEG_I64 19
/* layouts */
#define TRANSOAR_SEG_NCDHW 0
#define TRANSOAR_SEG_NDHWC 1

/* Bytes of `workspace` the head backward (C > 0) and the loss forward (any C) need at most, for every N and S. */
size_t transoar_seg_workspace_bytes(int C, int K);

/*
 * Head forward: y[v, k] = bias[k] + sum_c weight[k, c] * x[v, c].
 *   x       (N, C, D, H, W) in x_layout, dtype (F32 / BF16)
 *   weight  (K, C) fp32;  bias (K) fp32
 *   y       (N, K, D, H, W) channels-last (NDHWC), dtype
 */
int transoar_seg_head_forward(const void* x, int x_layout, int dtype, const float* weight, const float* bias, long N, long S, int C,
                              int K, void* y, void* hip_stream);

/*
 * Head backward.
 *   dy      (N, K, D, H, W) in dy_layout, dtype (the dtype of x)
 *   dx      (N, C, D, H, W) out in x_layout, dtype: dx[v, c] = sum_k weight[k, c] * dy[v, k];  NULL: not computed
 *   dw      (K, C) fp32 out: sum_v dy[v, k] * x[v, c];   db (K) fp32 out: sum_v dy[v, k]
 *   workspace  transoar_seg_workspace_bytes(C, K) bytes of device memory (the per-workgroup partial slabs)
 */
int transoar_seg_head_backward(const void* x, int x_layout, int dtype, const void* dy, int dy_layout, const float* weight, long N,
                               long S, int C, int K, void* dx, float* dw, float* db, float* workspace, void* hip_stream);

/*
 * Loss forward, one pass over the logits.
 *   logits  (N, K, D, H, W) in layout, dtype;  labels N * S integers of label_dtype;  fg_bg != 0: label -> (label > 0)
 *   losses  2 fp32 out: [segce, segdice]
 *   stats   2K fp32 out, kept for the backward: num_k = 2 tp_k + smooth_nom, den_k = P_k + Y_k + smooth_denom
 *           (tp_k = sum p_k [y = k], P_k = sum p_k, Y_k = sum [y = k] over batch and space; 2tp + fp + fn = P + Y)
 *   workspace  transoar_seg_workspace_bytes(0, K) bytes of device memory
 */
int transoar_seg_loss_forward(const void* logits, int layout, int dtype, const void* labels, int label_dtype, long N, long S, int K,
                              int fg_bg, float smooth_nom, float smooth_denom, float* losses, float* stats, float* workspace,
                              void* hip_stream);

/*
 * Loss backward: grad_logits (same shape, layout and dtype as logits) of g[0] * segce + g[1] * segdice, with g a DEVICE pointer
 * to the two upstream gradients:  d/dz_k = p_k (a_k - sum_j p_j a_j) + g[0] / (N S) (p_k - [y = k]),
 * a_k = -g[1] / (K - 1) (2 [y = k] / den_k - num_k / den_k^2) for k >= 1, a_0 = 0.
 */
int transoar_seg_loss_backward(const void* logits, int layout, int dtype, const void* labels, int label_dtype, long N, long S, int K,
                               int fg_bg, const float* stats, const float* g, void* grad_logits, void* hip_stream);

int transoar_segproxy_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
