/* C ABI of the model ensemble, exported by libunet_hip.so: the level-0 logits of several models (folds, seeds) for one volume are
 * turned into softmax probabilities one member at a time and folded into a running state whose size does not grow with the number
 * of members; a closing pass reads the state into the label map, the mean probabilities and two voxel-wise uncertainty maps.
 *
 * The reference trains and evaluates one network per run and has no counterpart.  The members, the state, the entropy and the
 * mutual information below are therefore this project's definitions: parity with TIPL is NOT pinned.
 *
 * MEMBERS  0..M-1, each a volume of level-0 logits {C, S}: fp32, plane c at logits + c*S (the offset is 64-bit), channel 0 the
 *   background, 2 <= C <= 65536, 1 <= S < 2^31.  Member m has a weight w_m > 0; the host normalises the weights in double so that
 *   they sum to 1 and passes each as fp32 (ensemble.normalize_weights).  Equal weights are 1/M; M = 1 gives exactly 1.0f.
 * PER MEMBER AND VOXEL  the online softmax state of the fused softmax pass of include/unet_postproc.h, taken over ascending c: the
 *   running maximum m, s = sum_c exp(x_c - m) and sf, the same over the foreground c >= 1.  Then
 *     d_c = x_c - m,  e_c = expf(d_c),  p_c = e_c / s,  fg = sf / s
 *   are that pass's own expressions, so an ensemble of one reproduces its probabilities bit for bit, and
 *     H_m = logf(s) - (sum_c e_c * d_c) / s
 *   summed over ascending c in fp32, a channel with x_c == -inf contributing 0: -sum_c p_c ln p_c with 0 ln 0 = 0, for one
 *   logarithm per voxel.  A bad voxel (a NaN logit, a +inf logit, or all channels -inf: that pass's rule) makes p, fg and H_m NaN.
 * STATE    {C+2, S} fp32: planes 0..C-1 hold sum_m w_m p_c, plane C holds sum_m w_m fg, plane C+1 holds sum_m w_m H_m.  Each sum
 *   runs over ascending m: the first member (first != 0) WRITES w_0 * value and never reads the state, which may hold anything;
 *   every later member adds w_m * value to what it reads.  Each product and each add is rounded in fp32 (no fused multiply-add), so
 *   the bits are the same on every run and for either load width.
 * FINALIZE with q_c = plane c:
 *     label_prob  {C-1, S} fp32   = planes 1..C-1
 *     fg_prob     {S} fp32        = plane C
 *     label       {S} uint16      = fg_prob > threshold ? 1 + argmax_{c >= 1} q_c : 0; the first index wins a tie, a comparison
 *                                   with NaN is false
 *     entropy     {S} fp32        = -sum_{c = 0..C-1} q_c * logf(q_c), ascending c in fp32, a term with q_c == 0 contributing 0:
 *                                   the entropy of the mean prediction in nats, in [0, ln C]; NaN follows the arithmetic
 *     mutual_info {S} fp32        = t < 0 ? 0 : t with t = entropy - plane C+1: the entropy of the mean minus the mean of the
 *                                   members' entropies, i.e. how much the members DISAGREE; NaN stays NaN
 *   entropy is high when the members disagree or when every member is unsure; mutual_info only in the first case.
 *   Each of the five outputs may be NULL (not written); at least one must be wanted.
 *
 * unet_ens_state_bytes  (C + 2) * S * 4, the bytes of the state.
 * unet_ens_accumulate   one streaming pass: reads the member's C planes (a second time from memory only beyond 8 channels),
 *   reads the C + 2 state planes unless first, writes them: 4 * S * (C + 2 * (C + 2)) bytes, 4 * S * (C + (C + 2)) when first.
 * unet_ens_finalize     one streaming pass: reads the state planes the wanted outputs need once, writes the wanted outputs.
 *
 * Any 4-byte pointer alignment works: 16-byte loads and stores are used when S % 4 == 0 and every pointer of the call is 16-byte
 * aligned (8 for the uint16 label), scalar ones otherwise, with the same bits.  Argument errors (NULL logits, state or bytes;
 * out_c outside [2, 65536]; voxels outside [1, 2^31); a weight that is not finite or not in (0, 1]; a state smaller than
 * unet_ens_state_bytes says; no output wanted) are found before any device call.  Both passes run on the caller's stream and need
 * nothing beyond the state.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_ENSEMBLE_H
#define UNET_ENSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int unet_ens_state_bytes(int out_c, int64_t voxels, size_t* bytes);

int unet_ens_accumulate(const float* logits, int out_c, int64_t voxels, float weight, int first, void* state, size_t state_bytes,
                        void* stream);

int unet_ens_finalize(const void* state, size_t state_bytes, int out_c, int64_t voxels, float threshold, float* label_prob,
                      float* fg_prob, uint16_t* label, float* entropy, float* mutual_info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
