// m3t_features.hip -- the built-in feature detector of TextureModality: what DetectAndComputeCorrKeypoints
// (M3T/src/texture_modality.cpp:858-888) asks of OpenCV, as a detector of the project's own (m3t_features.h;
// tests/feature_reference.py is its definition).  Three kernels on the context's stream, no host read between them:
//   texture_focus_kernel     (detector, row band)  region of interest from the device pose, grey + bilinear sample
//   texture_fast_kernel      (detector, row band)  FAST-9 score, 3 x 3 suppression, 5 x 5 box sums
//   texture_describe_kernel  (detector)            the n best corners in raster order, direction, descriptor, keypoints
// and their *_list_kernel forms for the detectors an enqueued call lists (m3t_hip_reset_bodies, m3t_hip_judge_bodies).
// Included by m3t_hip_api.hip behind m3t_texture.hip (same translation unit).

// (Included twice, like m3t_texture.hip: with M3T_TEXTURE_LIST_KERNELS defined it yields the three list kernels alone.)
#ifndef M3T_TEXTURE_LIST_KERNELS

typedef const __attribute__((address_space(4))) TextureDetectorDev CDetector;

__constant__ int16_t k_feature_cos[M3T_FEATURE_DIRECTIONS] = {M3T_FEATURE_COS_VALUES};
__constant__ int16_t k_feature_sin[M3T_FEATURE_DIRECTIONS] = {M3T_FEATURE_SIN_VALUES};
__constant__ int8_t k_feature_pattern[M3T_BRIEF_TESTS * 4] = {M3T_BRIEF_PATTERN_VALUES};

constexpr int kFeatureThreads = 256;           // focus and FAST kernels
constexpr int kDescribeThreads = 1024;         // one workgroup per detector
constexpr int kFastRows = M3T_FEATURE_BAND + 2 * M3T_FEATURE_FAST_HALO;  // image rows of a band in LDS
constexpr int kScoreRows = M3T_FEATURE_BAND + 2;                         // score rows of a band in LDS

extern "C" {

// (The three kernels' bodies live in m3t_features_focus.inc / _fast.inc / _describe.inc: the list kernels below include
// the same text behind their test, and these three compile to what they always were.)
__global__ void __launch_bounds__(kFeatureThreads)
texture_focus_kernel(const TextureDetectorDev* detectors, const TextureModDev* mods, const CameraDev* cams,
                     const float* body_poses) {
  const unsigned detector_index = blockIdx.x;
#include "m3t_features_focus.inc"
}

// A band of M3T_FEATURE_BAND rows with a halo of 4 (3 for the circle, 1 for the suppression) in LDS: 24 rows of 512
// bytes, and the scores of the band with a halo of 1: 18 rows of 512 u16 -- 30 KB.
__global__ void __launch_bounds__(kFeatureThreads)
texture_fast_kernel(const TextureDetectorDev* detectors) {
  const unsigned detector_index = blockIdx.x;
#include "m3t_features_fast.inc"
}

// Selection (score descending, raster index ascending; output in raster order), direction and descriptor.  LDS: the
// score histogram (4096 words), the kept corners' raster indices (4096 words) and a few words per wave: 33 KB.
// Every wave owns a contiguous piece of the raster, so the raster order of the output is a ballot within the wave and a
// prefix over the waves' counts; no atomic decides an order (the histogram's atomics only count).
__global__ void __launch_bounds__(kDescribeThreads)
texture_describe_kernel(const TextureDetectorDev* detectors) {
  const unsigned detector_index = blockIdx.x;
#include "m3t_features_describe.inc"
}

}  // extern "C"

#else  // M3T_TEXTURE_LIST_KERNELS

extern "C" {

// ---- StartModality (texture_modality.cpp:315-322) of the texture modalities an enqueued call lists ----
// items: {detector, texture modality, flag index or -1} per listed modality, three ints each, in the call's argument
// block; the item is blockIdx.x.  flags == nullptr (m3t_hip_reset_bodies): every item runs.  Otherwise
// (m3t_hip_judge_bodies: the judge's flags) item k runs iff flags[items[3 k + 2]] != 0.  The test is block-uniform and
// the three kernels here and texture_keyframe_list_kernel (m3t_texture.hip) form it from the same words -- the judge
// kernels wrote the flags before the first of them and nobody writes them in between -- so a modality is restarted by
// all four or by none.  A skipped item returns before its first store and its first barrier: its detector header,
// images, features, keyframes and state keep their bits.  (texture_item_skipped: m3t_texture.hip)
__global__ void __launch_bounds__(kFeatureThreads)
texture_focus_list_kernel(const TextureDetectorDev* detectors, const TextureModDev* mods, const CameraDev* cams,
                          const float* body_poses, const int* items, const int* flags) {
  if (texture_item_skipped(items, flags, (int)blockIdx.x)) return;  // block-uniform
  const int detector_index = items[3 * blockIdx.x];
#include "m3t_features_focus.inc"
}
__global__ void __launch_bounds__(kFeatureThreads)
texture_fast_list_kernel(const TextureDetectorDev* detectors, const int* items, const int* flags) {
  if (texture_item_skipped(items, flags, (int)blockIdx.x)) return;  // block-uniform
  const int detector_index = items[3 * blockIdx.x];
#include "m3t_features_fast.inc"
}
__global__ void __launch_bounds__(kDescribeThreads)
texture_describe_list_kernel(const TextureDetectorDev* detectors, const int* items, const int* flags) {
  if (texture_item_skipped(items, flags, (int)blockIdx.x)) return;  // block-uniform
  const int detector_index = items[3 * blockIdx.x];
#include "m3t_features_describe.inc"
}

}  // extern "C"

#endif  // M3T_TEXTURE_LIST_KERNELS
