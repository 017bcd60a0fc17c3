/*
 * transoar_patchmerge.h -- C ABI of the Swin encoder's convolutional patch merging: Conv3d(C, 2C, kernel 2, stride 2,
 * padding 0, no bias) on a channels-last token map (ConvPatchMerging, transoar/models/backbones/encoder_blocks.py).
 * Kernels: transoar_amd/csrc/patch_merge.hip; DESIGN.md section 12.15.
 *
 *     y[b, d', h', w', n] = sum_{kd, kh, kw, c} weight[n, c, kd, kh, kw] . x[b, 2 d' + kd, 2 h' + kh, 2 w' + kw, c]
 *
 * x / dx (B, D, H, W, C) bf16, y / dy (B, D/2, H/2, W/2, 2C) bf16 (extents rounded down: an odd extent drops its last
 * plane, row or column; dx is written as zeros there), all dense.  weight (2C, C, 2, 2, 2): fp32 (weight_dtype 0) or
 * bf16 (weight_dtype 2); d_weight the same layout in fp32.  `packed` (2C, 8C) bf16 is written by transoar_patch_merge_pack:
 * row n holds weight[n] reordered to [kd, kh, kw, c], the order in which the two voxels (2 w', 2 w' + 1) of an input line
 * lie in memory; forward and data gradient read it.
 * Workspace: transoar_patch_merge_workspace_bytes(what, ...) with what = 0 forward (fp32 partials of the split-K route),
 * 1 weight gradient (fp32 partials per group of lines; the reduce pass sums them in a fixed order: no atomics,
 * bit-stable).  The data gradient needs none.
 * Limits: C % 16 == 0, every extent >= 2, every buffer below 2^31 bytes.  Device pointers, 16-byte aligned; asynchronous
 * on `hip_stream`.  Returns 0, a hipError_t, or a negative code below; a negative code is returned before the first HIP
 * call.
 */
#ifndef TRANSOAR_PATCHMERGE_H
#define TRANSOAR_PATCHMERGE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
  TRANSOAR_PATCHMERGE_OK = 0,
  TRANSOAR_PATCHMERGE_ERR_NULL = -1,
  TRANSOAR_PATCHMERGE_ERR_DIM = -2,         /* C % 16 != 0, an extent below 2, a buffer of 2^31 bytes or more */
  TRANSOAR_PATCHMERGE_ERR_WORKSPACE = -3,
  TRANSOAR_PATCHMERGE_ERR_ALIGN = -4,
  TRANSOAR_PATCHMERGE_ERR_DTYPE = -5
};

size_t transoar_patch_merge_workspace_bytes(int what, int B, int D, int H, int W, int C);

int transoar_patch_merge_pack(const void* weight, int weight_dtype, void* packed, int C, void* hip_stream);

int transoar_patch_merge_forward(const void* x, const void* packed, void* y, void* workspace, size_t workspace_bytes,
                                 int B, int D, int H, int W, int C, void* hip_stream);

int transoar_patch_merge_dgrad(const void* dy, const void* packed, void* dx, int B, int D, int H, int W, int C,
                               void* hip_stream);

int transoar_patch_merge_wgrad(const void* x, const void* dy, float* d_weight, void* workspace, size_t workspace_bytes,
                               int B, int D, int H, int W, int C, void* hip_stream);

int transoar_patchmerge_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
