/*
 * transoar_augment.h -- C ABI of the batch augmentation for MI355X (gfx950): intensity range scaling, ONE trilinear resample of
 * the volume (nearest for its label map) through a per-sample affine map, and an intensity gain / offset, in one launch.
 *
 * What it stands in for: the train chain of transoar/data/transforms.py:76-165 (get_transforms) as the two shipped YAMLs switch it
 * on -- ScaleIntensityRanged, RandRotated, RandZoomd, RandAffined (translate), RandFlipd x 3, RandSpatialCropd,
 * RandScaleIntensityd, RandShiftIntensityd -- which the reference runs on host workers and which resamples the volume after every
 * spatial step.  Two deliberate differences: the spatial steps are composed into one map per sample (the table below) and the
 * volume is interpolated once, trilinear (the reference interpolates after every step and zooms in `area` mode); and the random
 * parameters come from this project's own seeded generator (transoar_amd/augment.py), not MONAI's stream.  Gaussian noise,
 * Gaussian smoothing, gamma contrast and shear (all off in both YAMLs) are not implemented.
 *
 * The operation.  params is (n, 16) fp32; row s holds, for sample s,
 *   slots 0..11   the rows of [M | t] (3 x 4): output INDEX o = (d, h, w) reads source index  src = M o + t  (centres and the
 *                 crop offset are folded into t on the host, in fp64, before rounding to fp32),
 *   slot 12       gain,   slot 13  offset,   slots 14..15  zero.
 * The table of a chain (transoar_amd/augment.py, compose_params), with S the INPUT extents, c = (S - 1) / 2, R = Rx Ry Rz the
 * rotation on (D, H, W), z the zoom, tr the translation in voxels, F = diag(+-1) and f = (S - 1 where flipped, else 0) the
 * flips, and k the crop offset -- the output -> source map is the product of the steps' maps in reverse chain order:
 *   M = (R / z) F,      t = c + (R / z) (F k + f - tr - c).
 * With v(x) = clamp((x - a_min) / (a_max - a_min), 0, 1) in fp32 (IEEE division):
 *   image_out = T(src) * gain + offset      (two roundings, no contraction)
 * where T is the trilinear interpolation of v over the eight corners floor(src) + {0,1}^3; a corner outside the volume
 * contributes 0 and is not read (neither is a corner of weight 0).  This is grid_sample(mode='bilinear', padding_mode='zeros',
 * align_corners=True) on the grid 2 src / (S - 1) - 1.
 *   labels_out = the label at floor(src + 0.5) per axis, or 0 outside the volume.
 * A source coordinate that is not finite or beyond +-2^24 counts as outside: that is decided in floating point before any
 * conversion to an integer, so no address outside the sample is ever formed.  src is computed in fp64 from the fp32 table
 * (FMAs, any order), floor and fraction are taken in fp64 and the fraction is then rounded to fp32: the weights carry one fp32
 * rounding each, not the rounding of a coordinate.  For tables with M in {0, +-1} and integral t every order and precision is
 * exact, and the outputs are bit-identical to the fp32 restatement (augment_torch).  The image is expected to be finite.
 *
 * One kernel writes both outputs.  A lane owns four consecutive outputs of a W row: with wout a multiple of 4 and 16-byte
 * aligned outputs the image leaves as one 16-byte store and the labels as one packed store; any other shape takes scalar stores.
 *
 * All pointers are device pointers.  Asynchronous on `hip_stream`; capturable (no host synchronisation, no host read of a device
 * value, no allocation).  Returns 0, a hipError_t (> 0), or a negative TRANSOAR_AUG_ERR_* code (checked on the host before any
 * launch, nothing printed).
 */
#ifndef TRANSOAR_AUGMENT_H
#define TRANSOAR_AUGMENT_H
#ifdef __cplusplus
extern "C" {
#endif

#define TRANSOAR_AUG_PARAMS 16           /* floats per row of the table */
#define TRANSOAR_AUG_MAX_EXTENT 16777216 /* 2^24: every index is exact in fp32 */
#define TRANSOAR_AUG_ERR_NULL (-1)       /* a required pointer is NULL, or only one of labels / labels_out is given */
#define TRANSOAR_AUG_ERR_DIM (-2)
#define TRANSOAR_AUG_ERR_DTYPE (-3)      /* unknown label dtype */
#define TRANSOAR_AUG_ERR_ALIGN (-4)      /* a pointer not aligned to its element type */

/* label types (the codes of transoar_boxtargets.h) */
#define TRANSOAR_AUG_U8 16
#define TRANSOAR_AUG_I16 17
#define TRANSOAR_AUG_I32 18
#define TRANSOAR_AUG_I64 19

/*
 *   image       (n, di, hi, wi) contiguous fp32 ((n, 1, di, hi, wi) is the same memory)
 *   labels      NULL, or (n, di, hi, wi) contiguous integers of label_dtype
 *   params      (n, 16) fp32, see above
 *   image_out   (n, dout, hout, wout) fp32 out
 *   labels_out  NULL exactly when labels is; (n, dout, hout, wout) of label_dtype out
 * TRANSOAR_AUG_ERR_DIM: an extent < 1, an output extent above the input's, an input extent above TRANSOAR_AUG_MAX_EXTENT,
 * n > 65535, a sample of 2^40 voxels or more, an output sample of 2^33 voxels or more, or a_min / a_max not finite or
 * a_max <= a_min.
 */
int transoar_augment_forward(const float* image, const void* labels, int label_dtype, int n, int di, int hi, int wi, int dout,
                             int hout, int wout, const float* params, float a_min, float a_max, float* image_out,
                             void* labels_out, void* hip_stream);

int transoar_augment_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
