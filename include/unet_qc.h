/* C ABI of quality control (qc.cpp:55-160), exported by libunet_hip.so.
 *
 * unet_qc_counts is the per-voxel half of calculate_qc (qc.cpp:86-135) plus shift_subject_label (train.cpp:248-256) in one pass
 * over the engine's level-0 output, on the caller's stream:
 *   shift   (shift_by > 0 only)  l = label != 0 ? label + shift_by : (image0 > 0 ? 1 : 0), in float
 *   cast    t = (int64)l, toward zero (.to(torch::kLong), qc.cpp:86)
 *   valid   0 <= t < out_c (qc.cpp:103)
 *   collapse (collapse_before = k > 0, qc.cpp:105-117): candidates [logsumexp(l_0..l_{k-1}), l_k, .., l_{out_c-1}],
 *           t' = max(t - k + 1, 0), C' = out_c - k + 1; without collapse t' = t, C' = out_c
 *   argmax  torch.argmax's rules: the first index wins a tie, a NaN is the maximum (the first NaN wins)
 *   counts  a valid voxel adds 1 to voxels[t'], and 1 to wrong[t'] when argmax != t'; invalid voxels count nowhere
 * counts (uint64, 2*C'): voxels[0..C') then wrong[0..C').  It is WRITTEN, not accumulated.
 *
 * Volumes are fp32 device arrays: logits {out_c, voxels} (NCDHW of outs[0], unet_hip.h), label {voxels}, image0 {voxels} (input
 * channel 0; read only when shift_by > 0, may be NULL otherwise).  Any alignment and any voxel count work.  All scratch is the
 * caller's (unet_qc_scratch_bytes): calls on different streams with different scratch may run concurrently.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_QC_H
#define UNET_QC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int unet_qc_scratch_bytes(int out_c, int64_t voxels, int collapse_before, size_t* bytes);
int unet_qc_counts(const float* logits, const float* label, const float* image0, int out_c, int64_t voxels, int collapse_before,
                   int shift_by, uint64_t* counts, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
