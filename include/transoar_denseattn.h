/*
 * transoar_denseattn.h -- C ABI of the dense multi-head cross-attention of the Focused Decoder at head dimension 48
 * (FocusedAttn.forward without the RoI gather: restrict_attn False, or attention volumes too large to gather;
 * transoar/models/necks/focused_decoder.py:228-262).  Kernels: transoar_amd/csrc/dense_attn.hip.
 *
 * Per (batch element b, head h), C = 384, H = 8, hd = 48:
 *
 *     S    = scale . Q[b, :, 48 h : 48 h + 48] . K[b, :, 48 h : 48 h + 48]^T        (Nq x L)
 *     S[r, j] = -inf where bit j of keybits[organ(r)] is set                        organ(r) = r / rows_per_organ
 *     O    = softmax_rows(S) . V[b, :, 48 h : 48 h + 48]                            lse[b, h, r] = log sum exp of row r
 *   backward:  P = exp(S - lse),  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - rowsum(dO o O)),
 *     dQ   = scale . dS K,   dK = scale . dS^T Q
 *
 * Q / O / dO / dQ (B, Nq, C) bf16, K / V / dK / dV (B, L, C) bf16, row-major and dense; a head is the 48-column slice
 * of its token matrix, read and written in place (no (B, H, N, hd) copies, nothing padded to 64).  lse (B, H, Nq) fp32,
 * natural logarithm.
 * keybits (O, ceil(L / 32)) uint32 or NULL (nothing masked): bit i of word t = key 32 t + i is masked; the bits of keys
 * >= L must be set (the kernels also mask those keys themselves).  bounds (O, 2) int32, required with keybits:
 * [first 32-key tile that holds a live key, last such tile + 1) of each organ -- tiles outside are skipped unread, so a
 * live key outside its organ's bounds is ignored.  With keybits, Nq == O * rows_per_organ.  An organ without a live
 * key is outside the contract (the reference yields NaN): the caller must not pass one.
 * n_split: the keys are divided among n_split workgroups in the forward and in the dQ kernel, partial results in
 * `workspace` (transoar_dense_attn_workspace_bytes; the backward also keeps rowsum(dO o O) there); results do not
 * depend on it beyond fp32 rounding.  dK / dV are owned by one workgroup per (b, h, 64 keys): no atomics, bit-stable.
 * Limits: C == 384, H == 8, 1 <= n_split <= 64, every buffer below 2^31 bytes.  Device pointers, 16-byte aligned;
 * asynchronous on `hip_stream`.  Returns 0, a hipError_t, or a negative code below; a negative code is returned
 * before the first HIP call.
 */
#ifndef TRANSOAR_DENSEATTN_H
#define TRANSOAR_DENSEATTN_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
  TRANSOAR_DENSEATTN_OK = 0,
  TRANSOAR_DENSEATTN_ERR_NULL = -1,
  TRANSOAR_DENSEATTN_ERR_DIM = -2,          /* C != 384, H != 8, Nq != O * rows_per_organ, a size out of range */
  TRANSOAR_DENSEATTN_ERR_WORKSPACE = -3,
  TRANSOAR_DENSEATTN_ERR_ALIGN = -4
};

size_t transoar_dense_attn_workspace_bytes(int B, int Nq, int n_split);

int transoar_dense_attn_forward(const void* q, const void* k, const void* v, const unsigned* keybits, const int* bounds,
                                void* o, float* lse, void* workspace, size_t workspace_bytes, int B, int Nq, long L, int C,
                                int H, int O, int rows_per_organ, float scale, int n_split, void* hip_stream);

int transoar_dense_attn_backward(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                                 const float* lse, const unsigned* keybits, const int* bounds, void* dq, void* dk, void* dv,
                                 void* workspace, size_t workspace_bytes, int B, int Nq, long L, int C, int H, int O,
                                 int rows_per_organ, float scale, int n_split, void* hip_stream);

int transoar_denseattn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
