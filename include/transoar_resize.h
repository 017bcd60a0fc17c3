/*
 * transoar_resize.h -- C ABI of the case resize for MI355X (gfx950): an adaptive-average ("area") resize of a volume and torch's
 * nearest rule for its label map, both read through a per-sample crop window and written as a crop of the resized grid, in one
 * launch; and the foreground window of a label map (two launches), which stays on the device and feeds the resize.
 *
 * What it stands in for: CropForegroundd followed by Resized(mode=['area', 'nearest']) of transoar/data/transforms.py:37-75
 * (transform_preprocessing_amos / _visceral), and the ScaleIntensityRanged -> Resized -> RandSpatialCropd head of the 'test'
 * chain of get_transforms.  MONAI is not installed where this was written.  Two things therefore rest on reading MONAI 0.7 from
 * memory and are NOT checked against it: (1) that Resized calls torch.nn.functional.interpolate with the given mode on the whole
 * array (interpolate IS installed: on CPU tensors it is the reference of the tests, and the rules below were checked against it);
 * (2) the clipped margin rule of CropForegroundd stated under "Foreground window".
 *
 * Window.  window is NULL (the whole volume, crop 0) or (n, 12) int32; row s holds, for sample s, on (D, H, W):
 *   slots 0..2  start,   slots 3..5  extent,   slots 6..8  crop,   slot 9  found (not read by the resize),   slots 10..11  zero.
 * The kernel clamps every row before use -- start into [0, S - 1], extent into [1, S - start], crop into [0, R - out], with S the
 * source extents, R the resized grid and out the output extents -- so no address outside the sample is ever formed, whatever
 * the table holds.
 *
 * Area (image).  With E the window's extent and R the resized grid (host arguments), index o of the resized grid averages the
 * window-relative source indices [floor(o E / R), ceil((o + 1) E / R)) on each axis, in exact integer arithmetic: the fp32 sum of
 * the bin (in a fixed order) divided (IEEE) by its count.  No atomics: the same input gives the same bits.
 * This is F.interpolate(mode='area') = adaptive_avg_pool3d, E < R (bins of one or two voxels) included.  With scale_range != 0
 * every voxel is first mapped to v = clamp((x - a_min) / (a_max - a_min), 0, 1) in fp32 (IEEE division).  The image is fp32 or
 * int16 (what a CT file holds); the output is fp32.
 *
 * Nearest (labels).  The source index is min((int)floorf((float)o * ((float)E / (float)R)), E - 1), in fp32 as torch computes
 * it -- NOT the exact integer quotient o E / R, from which it differs on 74 of the pairs E, R in 1..96 (26 -> 22, 39 -> 33, ...).
 * The output has the labels' type.
 *
 * Crop.  The kernel writes the indices o in [crop, crop + out) of the resized grid, out <= R; with out == R the plain resize.
 *
 * Foreground window.  Per sample, lo / hi = the smallest / largest index per axis of the voxels whose label is selected: bit c
 * of class_mask selects class c (1..62); a negative class_mask selects every label > 0.  Then start = max(lo - margin, 0),
 * end = min(hi + 1 + margin, S), and the whole row is written: extent = end - start, crop = 0, found = 1.  With no selected voxel
 * the row is the whole volume and found = 0.  (MONAI 0.7's CropForegroundd clips the margin at the border like this, as read
 * from memory; see above.)  Integer minima and maxima only: bit-reproducible.  Every workspace word that is read was written by
 * the same call.
 *
 * All pointers are device pointers.  Asynchronous on `hip_stream`; capturable (no host synchronisation, no host read of a device
 * value, no allocation).  Returns 0, a hipError_t (> 0), or a negative TRANSOAR_RSZ_ERR_* code (checked on the host before any
 * launch, nothing printed).
 */
#ifndef TRANSOAR_RESIZE_H
#define TRANSOAR_RESIZE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TRANSOAR_RSZ_WINDOW 12           /* ints per row of the window table */
#define TRANSOAR_RSZ_MAX_EXTENT 16777216 /* 2^24: every index is exact in fp32 */
#define TRANSOAR_RSZ_ERR_NULL (-1)       /* a required pointer is NULL, or only one of labels / labels_out is given */
#define TRANSOAR_RSZ_ERR_DIM (-2)
#define TRANSOAR_RSZ_ERR_DTYPE (-3)      /* unknown image or label dtype */
#define TRANSOAR_RSZ_ERR_ALIGN (-4)      /* a pointer not aligned to its element type */
#define TRANSOAR_RSZ_ERR_WORKSPACE (-5)  /* workspace_bytes below transoar_foreground_window_workspace_bytes */

/* image types */
#define TRANSOAR_RSZ_F32 0
/* label types (the codes of transoar_boxtargets.h); TRANSOAR_RSZ_I16 is also an image type */
#define TRANSOAR_RSZ_U8 16
#define TRANSOAR_RSZ_I16 17
#define TRANSOAR_RSZ_I32 18
#define TRANSOAR_RSZ_I64 19

/*
 *   image       (n, di, hi, wi) contiguous, fp32 or int16 by image_dtype ((n, 1, di, hi, wi) is the same memory)
 *   labels      NULL, or (n, di, hi, wi) contiguous integers of label_dtype
 *   rd, rh, rw  the resized grid R;   dout, hout, wout <= R  the part of it that is written
 *   window      NULL, or (n, 12) int32, see above
 *   image_out   (n, dout, hout, wout) fp32 out
 *   labels_out  NULL exactly when labels is; (n, dout, hout, wout) of label_dtype out
 * TRANSOAR_RSZ_ERR_DIM: an extent < 1 or above TRANSOAR_RSZ_MAX_EXTENT, out > R on an axis, n > 65535, a sample of 2^40 voxels
 * or more, an output sample of 2^33 voxels or more, or, with scale_range != 0, a_min / a_max not finite or a_max <= a_min.
 */
int transoar_resize_forward(const void* image, int image_dtype, const void* labels, int label_dtype, int n, int di, int hi, int wi,
                            int rd, int rh, int rw, int dout, int hout, int wout, const int* window, int scale_range, float a_min,
                            float a_max, float* image_out, void* labels_out, void* hip_stream);

/*
 *   labels      (n, sd, sh, sw) contiguous integers of label_dtype
 *   class_mask  bit c selects class c (1..62); negative: every label > 0
 *   margin_*    >= 0, at most TRANSOAR_RSZ_MAX_EXTENT
 *   window      (n, 12) int32 out, every slot written
 *   workspace   transoar_foreground_window_workspace_bytes(n, sd * sh * sw) bytes, 4-byte aligned; contents need not be set
 */
int transoar_foreground_window(const void* labels, int label_dtype, int n, int sd, int sh, int sw, long class_mask, int margin_d,
                               int margin_h, int margin_w, int* window, void* workspace, size_t workspace_bytes, void* hip_stream);

/* 0 for dimensions transoar_foreground_window refuses */
size_t transoar_foreground_window_workspace_bytes(int n, long voxels_per_sample);

int transoar_resize_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
