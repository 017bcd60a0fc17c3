/*
 * transoar_boxtargets.h -- C ABI of the detection targets from label volumes for MI355X (gfx950): per sample and organ class
 * the bounding box of the class's voxels, padded, normalised and in centre / size form, as the dense targets of the set criterion.
 *
 * Reference semantics: transoar/utils/bboxes.py:45-96, segmentation2bbox(labels, padding, 'cxcyczwhd', normalize=True), which the
 * reference's collator runs on the host for every batch (transoar/data/dataloader.py:56).  For sample s and class c in 1..k, with
 * lo[a] / hi[a] the smallest / largest index of a voxel with label c along tensor axis 1 + a (box axes x, y, z = D, H, W):
 *   the class is absent when it has no voxel or hi[a] - lo[a] < min_extent on any axis (the reference hard-codes 5); otherwise,
 *   in fp32 and in this order,  lo = max(lo - padding, 0), hi = min(hi + padding, size)  (size, not size - 1),
 *   lo /= size, hi /= size,  (w, h, d) = hi - lo,  (cx, cy, cz) = (hi + lo) / 2.
 * With IEEE fp32 division the boxes are bit-identical to the reference's.
 *
 * One deliberate difference: labels that are 0, negative or above k are ignored.  The reference would emit a box for a class
 * above k; the dense targets (N, k, 6) have no slot for it.
 *
 * Two launches.  The first gives every 256-thread workgroup a contiguous run of one sample's voxels, read 16 bytes per lane; the
 * workgroup keeps a k x 6 table of integer minima / maxima in LDS (integer LDS atomics, after a lane has collapsed the runs of
 * equal labels in its 16 bytes) and stores it as one row of `workspace`.  The second reduces the rows and applies the rule above.
 * Integer minima and maxima only: the result is bitwise reproducible, and every workspace word that is read has been written
 * by the first launch, so it does not depend on what the workspace held before.
 *
 * All pointers are device pointers; `labels` is aligned to its element size.  Asynchronous on `hip_stream`; capturable (no host
 * synchronisation, no host read of a device value).  Returns 0, a hipError_t (> 0), or a negative TRANSOAR_BOX_ERR_* code
 * (checked on the host before any launch, nothing printed).
 */
#ifndef TRANSOAR_BOXTARGETS_H
#define TRANSOAR_BOXTARGETS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TRANSOAR_BOX_MAX_K 64
#define TRANSOAR_BOX_ERR_NULL (-1)
#define TRANSOAR_BOX_ERR_DIM (-2)
#define TRANSOAR_BOX_ERR_DTYPE (-3)      /* unknown label dtype, or a workspace that is too small */
#define TRANSOAR_BOX_ERR_ALIGN (-4)      /* labels not aligned to the label type */

/* label types (the codes of transoar_segproxy.h) */
#define TRANSOAR_BOX_U8 16
#define TRANSOAR_BOX_I16 17
#define TRANSOAR_BOX_I32 18
#define TRANSOAR_BOX_I64 19

/* Bytes of `workspace` for n samples of voxels_per_sample voxels and k classes; 0 for arguments the forward would refuse. */
size_t transoar_box_targets_workspace_bytes(int n, long voxels_per_sample, int k);

/*
 *   labels     (n, sx, sy, sz) contiguous integers of label_dtype ((n, 1, sx, sy, sz) is the same memory)
 *   boxes      (n, k, 6) fp32 out: cx cy cz w h d, normalised; zeros where the class is absent
 *   present    (n, k) bytes out: 1 / 0
 *   counts     2 fp32 out: [num_boxes, n_present] (equal: one box per present class)
 *   workspace  at least transoar_box_targets_workspace_bytes(n, sx * sy * sz, k) bytes, 4-byte aligned; contents irrelevant
 * TRANSOAR_BOX_ERR_DIM: n, sx, sy or sz < 1, n > 65535, k outside 1..TRANSOAR_BOX_MAX_K, padding < 0, min_extent < 0, or a
 * sample of 2^40 voxels or more.
 */
int transoar_box_targets_forward(const void* labels, int label_dtype, int n, int sx, int sy, int sz, int k, int padding,
                                 int min_extent, float* boxes, unsigned char* present, float* counts, void* workspace,
                                 size_t workspace_bytes, void* hip_stream);

int transoar_boxtargets_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
