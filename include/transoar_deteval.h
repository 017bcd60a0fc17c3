/*
 * transoar_deteval.h -- C ABI of the detection records of a validation pass for MI355X (gfx950): per image and organ class the
 * one detection the reference decodes, and its IoU with the class's ground-truth box, appended to device buffers.
 *
 * Reference semantics: transoar/inference.py (the query of an organ with the largest sigmoid probability is its detection,
 * score = that probability) and the IoU the reference's DetectionEvaluator computes for it (transoar/utils/bboxes.py:150-186,
 * iou_3d_np after box_cxcyczwhd_to_xyzxyz).  With one detection per class and at most one ground-truth box per class the
 * evaluator's matching needs nothing but (score, IoU, has_gt) per (image, class); the precision / recall arithmetic runs once
 * per validation pass on the host (transoar_amd/evaluation.py::detection_metrics).
 *
 * Rule per (image s, class c), queries q = c * qpo + j, j in 0..qpo-1:
 *   p_j = 1 / (1 + expf(-x_j)) in fp32; the chosen query has the largest p_j (probabilities are compared, not logits), the
 *   lowest j among equals; a NaN never wins over a number (all NaN: j = 0).  score = p_j, box = the chosen row as fp32.
 *   gt_present: with (x1, y1, z1, x2, y2, z2) = (c - 0.5 * size, c + 0.5 * size) of both boxes, v = dx * dy * dz (left to
 *   right), inter = max(min(x2) - max(x1), 0) * ..., union = (v1 + v2) - inter, iou = inter / union: fp32, no contraction, one
 *   IEEE division -- bit-identical to numpy's.  Otherwise iou = -1 and has_gt = 0.
 * The records of image s go to row cursor + s of the record arrays.
 *
 * ONE launch of ONE workgroup of 256 threads: its four waves stride over the n * k (image, class) pairs, the lanes over the
 * qpo queries, and the wave reduces on (probability, index).  Every wave reads the cursor before it does any work; after a
 * barrier thread 0 stores cursor + n and threads < n_losses add losses[j] to loss_sums[j] in fp64.  When cursor + n > capacity
 * nothing is written except overflow = 1, and no address outside the arrays is formed.  Plain loads and stores, no atomics:
 * bitwise reproducible.
 *
 * All pointers are device pointers, aligned to their element type.  Asynchronous on `hip_stream`; capturable (no host
 * synchronisation, no host read of a device value).  Returns 0, a hipError_t (> 0), or a negative TRANSOAR_DETEVAL_ERR_* code
 * (checked on the host before any launch, nothing printed).
 */
#ifndef TRANSOAR_DETEVAL_H
#define TRANSOAR_DETEVAL_H
#ifdef __cplusplus
extern "C" {
#endif

#define TRANSOAR_DETEVAL_MAX_K 64
#define TRANSOAR_DETEVAL_MAX_QPO 4096
#define TRANSOAR_DETEVAL_MAX_N 1024
#define TRANSOAR_DETEVAL_MAX_LOSSES 32
#define TRANSOAR_DETEVAL_MAX_CAPACITY (1 << 20)
#define TRANSOAR_DETEVAL_ERR_NULL (-1)
#define TRANSOAR_DETEVAL_ERR_DIM (-2)
#define TRANSOAR_DETEVAL_ERR_DTYPE (-3)
#define TRANSOAR_DETEVAL_ERR_ALIGN (-4)

/* dtype of logits and boxes (the codes of transoar_msda3d.h) */
#define TRANSOAR_DETEVAL_F32 0
#define TRANSOAR_DETEVAL_BF16 2
#define TRANSOAR_DETEVAL_F16 3

/*
 *   logits      (n, k * qpo, 1) and boxes (n, k * qpo, 6), contiguous, both of `dtype`
 *   gt_boxes    (n, k, 6) fp32 cx cy cz w h d; gt_present (n, k) bytes, non-zero = the class has a box
 *   losses      n_losses fp32 values added to loss_sums (fp64[n_losses]); losses NULL or n_losses 0: nothing is added
 *   state       2 int32: {cursor, overflow}; capacity: rows (images) of the record arrays
 *   rec_score, rec_iou (capacity, k) fp32; rec_has_gt (capacity, k) bytes; rec_query (capacity, k) int32 (j within the organ);
 *   rec_box (capacity, k, 6) fp32
 * TRANSOAR_DETEVAL_ERR_DIM: k outside 1..64, qpo outside 1..4096, n outside 1..1024, n_losses outside 0..32 or capacity outside
 * 1..2^20.  TRANSOAR_DETEVAL_ERR_NULL: a NULL array (loss_sums only counts when losses are given).
 */
int transoar_deteval_accumulate(const void* logits, const void* boxes, int dtype, const float* gt_boxes,
                                const unsigned char* gt_present, const float* losses, int n_losses, int n, int k, int qpo,
                                int* state, int capacity, float* rec_score, float* rec_iou, unsigned char* rec_has_gt,
                                int* rec_query, float* rec_box, double* loss_sums, void* hip_stream);

int transoar_deteval_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
