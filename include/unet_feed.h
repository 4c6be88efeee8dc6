/* C ABI of the template/subject training feed (train.cpp:229-486,615-617), exported by libunet_hip.so.
 *
 * The per-sample label work of the reference's reader thread, on the device and on the caller's stream:
 *   unet_feed_label_max  max of the label read as int (read_label_info, train.cpp:229-246: tipl::image<3,int>, toward zero)
 *   unet_feed_prepare    in place, in the reader's order (train.cpp:415-419):
 *                          normalize (normalize != 0, !param.is_label)  l = l / max(l) when max(l) > 0 (tipl::normalize)
 *                          shift     (shift_by > 0, shift_subject_label train.cpp:248-257)
 *                                    l = l != 0 ? l + shift_by : (image0 > 0 ? 1 : 0), in float
 *   unet_feed_target     target = (int64)l, toward zero (.to(torch::kLong), train.cpp:615-617), after l / max(l) when normalize
 *                        != 0 (the out_count == 1 rule of the test set, train.cpp:373-374)
 * and the reference's sample schedule (train.cpp:391-401), host code.
 *
 * Volumes are fp32 device arrays of `voxels` values: label, image0 (input channel 0; read only when shift_by > 0, may be NULL
 * otherwise); target is int64.  Any alignment and any voxel count work.  The max is taken on the device (NaN voxels are skipped)
 * and never read back by the library.  All scratch is the caller's (unet_feed_scratch_bytes, the same size for every call on a
 * volume of that many voxels): calls on different streams with different scratch may run concurrently.
 *
 * Status codes / errors as in unet_hip.h (0 = ok, the message is read with unet_last_error).
 */
#ifndef UNET_FEED_H
#define UNET_FEED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int unet_feed_scratch_bytes(int64_t voxels, size_t* bytes);

/* *out_max (device int32) = max over the voxels of (int)label, clamped to the int range (INT_MIN when every voxel is NaN) */
int unet_feed_label_max(const float* label, int64_t voxels, int32_t* out_max, void* scratch, size_t scratch_bytes, void* stream);

/* label_max (device int32, may be NULL): receives unet_feed_label_max of the label as it was before this call */
int unet_feed_prepare(const float* image0, float* label, int64_t voxels, int normalize, int shift_by, int32_t* label_max,
                      void* scratch, size_t scratch_bytes, void* stream);

int unet_feed_target(const float* label, int64_t voxels, int normalize, int64_t* target, void* scratch, size_t scratch_bytes,
                     void* stream);

/* The cases the reader thread picks for seed_id in [first, first + count) (train.cpp:391-401):
 *   std::uniform_int_distribution<int> template_gen(0, max(1, n_template) - 1), non_template_gen(0, max(1, n_subject) - 1);
 *   std::mt19937 gen(seed);
 *   use_template = n_subject == 0 || seed_id % batch_size < n_template;
 *   case = use_template ? template_gen(gen) : non_template_gen(gen);          one draw per seed_id from 0, skipped ones included
 * with the C++ library's own std::mt19937 and std::uniform_int_distribution.  out_case[i] is the position in the template list
 * (out_is_template[i] = 1) or in the subject list (0) of seed_id first + i.  Host arrays of `count` entries. */
int unet_feed_schedule(uint64_t seed, int batch_size, int n_template, int n_subject, int64_t first, int64_t count, int32_t* out_case,
                       int32_t* out_is_template);

#ifdef __cplusplus
}
#endif
#endif
