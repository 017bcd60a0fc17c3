/*
 * transoar_augment.h -- C ABI of the batch augmentation for MI355X (gfx950): intensity range scaling, ONE trilinear resample of
 * the volume (nearest for its label map) through a per-sample affine map, and an intensity gain / offset, in one launch.
 *
 * What it stands in for: the train chain of transoar/data/transforms.py:76-165 (get_transforms) as the two shipped YAMLs switch it
 * on -- ScaleIntensityRanged, RandRotated, RandZoomd, RandAffined (translate), RandFlipd x 3, RandSpatialCropd,
 * RandScaleIntensityd, RandShiftIntensityd -- which the reference runs on host workers and which resamples the volume after every
 * spatial step.  Two deliberate differences: the spatial steps are composed into one map per sample (the table below) and the
 * volume is interpolated once, trilinear (the reference interpolates after every step and zooms in `area` mode); and the random
 * parameters come from this project's own seeded generator (transoar_amd/augment.py), not MONAI's stream.  The four steps that
 * both YAMLs switch off are here too: shear is one more factor of the map (below), and RandGaussianNoised, RandGaussianSmoothd
 * and RandAdjustContrastd are the intensity tail, transoar_augment_intensity (further below).
 *
 * The operation.  params is (n, 16) fp32; row s holds, for sample s,
 *   slots 0..11   the rows of [M | t] (3 x 4): output INDEX o = (d, h, w) reads source index  src = M o + t  (centres and the
 *                 crop offset are folded into t on the host, in fp64, before rounding to fp32),
 *   slot 12       gain,   slot 13  offset,   slots 14..15  zero.
 * The table of a chain (transoar_amd/augment.py, compose_params), with S the INPUT extents, c = (S - 1) / 2, R = Rx Ry Rz the
 * rotation on (D, H, W), z the zoom, tr the translation in voxels, F = diag(+-1) and f = (S - 1 where flipped, else 0) the
 * flips, and k the crop offset -- the output -> source map is the product of the steps' maps in reverse chain order:
 *   M = (R / z) F,      t = c + (R / z) (F k + f - tr - c).
 * With a shear S = I + (s01, s02, s10, s12, s20, s21) off the diagonal, applied between the translation and the flips:
 *   M = (R / z) S F,    t = c + (R / z) (S (F k + f - c) - tr).
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
 * One kernel writes both outputs of the resample.  A lane owns four consecutive outputs of a W row: with wout a multiple of 4 and 16-byte
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

/*
 * The intensity tail: what the reference's chain does to the cropped volume after the spatial steps, in the reference's order
 *   noise -> smooth -> gain -> offset -> gamma contrast
 * on image (n, d, h, w) fp32, per sample s from row s of `table`, (n, 12) 32-bit words:
 *   word 0       flags, uint32: TRANSOAR_AUG_NOISE | TRANSOAR_AUG_SMOOTH | TRANSOAR_AUG_CONTRAST
 *   word 1, 2    noise mean, noise std                       words 3..5  sigma_d, sigma_h, sigma_w
 *   word 6, 7    gain, offset                                word 8      gamma
 *   word 9, 10   the noise key k0, k1, uint32 (any bits)     word 11     zero
 * Every other word is fp32.  A step runs for a sample when its flag is set in the row AND in `steps`, and its parameters are
 * valid: noise needs a finite mean and std; smoothing needs all three sigmas in (0, 4] (a NaN is not); contrast needs a finite
 * gamma > 0.  A gain that is not finite counts as 1, such an offset as 0.  A step that does not run leaves the values as they
 * are, bit for bit (so does gain 1 with offset 0).  No table content can make a kernel form an index outside its arrays.
 *
 * Noise.  Voxel i (its linear index inside the sample) takes z = word (i & 3) of call j = i >> 2 of the normal generator:
 * Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl increments 0x9E3779B9, 0xBB67AE85) with key (k0, k1) on the counter
 * (j lo, j hi, 0, 0) gives r0..r3;  u1 = ((r0 >> 9) + 0.5) 2^-23,  u2 = (r1 >> 9) 2^-23  (both exact in fp32),
 * z0 = sqrt(-2 ln u1) cos(2 pi u2),  z1 = sqrt(-2 ln u1) sin(2 pi u2),  and z2, z3 the same from r2, r3.  v <- v + (mean + std z),
 * with the accurate logf, sincospif and sqrtf.
 *
 * Smoothing, MONAI's GaussianFilter(approx='erf', truncated=4): per axis  tail = int(max(4 sigma, 0.5) + 0.5)  in fp32 (at most
 * 16), the taps x = -tail..tail weigh  max(0.5 (erf(t (x + 0.5)) - erf(t (x - 0.5))), 0)  with t = 0.70710678 / sigma, divided
 * by their sum (computed in fp64, rounded to fp32 once).  The axes are filtered one after another with zero padding: a tap
 * outside the sample contributes 0 (and carries no noise).
 *
 * Gain and offset:  v <- v * gain + offset  (two roundings).
 *
 * Contrast, MONAI's AdjustContrast: with min and max over the sample at this point and r = max - min,
 *   v <- ((v - min) / (r + 1e-7))^gamma * r + min      (accurate powf; fp32 throughout).
 *
 *   image       (n, d, h, w) contiguous fp32           image_out  the same shape; may be `image` itself
 *   scratch     (n, d, h, w) fp32, distinct from both; may be NULL when `steps` has no TRANSOAR_AUG_SMOOTH
 *   steps       the union of the flags a row may carry: the passes of the others are not launched, their row flags ignored
 *   workspace   transoar_augment_intensity_workspace_bytes(n) bytes, 4-byte aligned; initialised by the call itself
 * With TRANSOAR_AUG_SMOOTH in `steps` the image makes two read-write passes (image -> scratch: noise and the H and W filters
 * of a tile staged in LDS; scratch -> image_out: the D filter, gain, offset, min / max), otherwise one; contrast adds one in
 * place.  The min / max reduction stays on the device (integer atomics on an order-preserving encoding, in the workspace).
 * TRANSOAR_AUG_ERR_NULL: image, image_out, table or workspace is NULL, or scratch is with TRANSOAR_AUG_SMOOTH in `steps`.
 * TRANSOAR_AUG_ERR_DIM: an extent < 1 or above TRANSOAR_AUG_MAX_EXTENT, n > 65535, or a sample of about 2^33 voxels or more.
 * TRANSOAR_AUG_ERR_ALIGN: a pointer that is not 4-byte aligned.  16-byte loads and stores are used when w % 4 == 0 and image,
 * image_out and scratch are 16-byte aligned, scalar ones with a masked row tail otherwise.
 */
#define TRANSOAR_AUG_TAIL_WORDS 12
#define TRANSOAR_AUG_NOISE 1
#define TRANSOAR_AUG_SMOOTH 2
#define TRANSOAR_AUG_CONTRAST 4
#define TRANSOAR_AUG_MAX_SIGMA 4

long transoar_augment_intensity_workspace_bytes(int n);
int transoar_augment_intensity(const float* image, float* image_out, float* scratch, int n, int d, int h, int w, const void* table,
                               int steps, void* workspace, void* hip_stream);

int transoar_augment_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
