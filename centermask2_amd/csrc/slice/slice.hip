// Sliced inference (TEST.SLICE, modeling/sliced_inference.py): the detections of every pass -- T tiles cut from one large image, each run
// at the model's own test size, and optionally the whole image as pass T -- mapped from the frame of the resized pass back into the frame
// of the image and written as ONE candidate set for cmk_nms_topk_metric (include/cmk.h).
//
//   slice_boxes_to_image_kernel   grid (ceil(K / 256), A), a thread per padded detection slot (a, k).  The row of the per-pass table
//                                 (x0, y0, rx, ry, tw, th) is uniform over a workgroup; the A clamped counts are read by every thread as
//                                 uniform loads to find the slot's place in the compacted output.  Latency-bound: A*K is a few thousand
//                                 rows of 36 bytes in and 40 out.
// Every step is one rounded fp32 operation (scale, then shift, then the clip): the tests restate it in numpy bit for bit, so nothing here
// may be contracted into an fma.  Every store is an ordinary vector store.
#include "cmk_common.hpp"

#include <math.h>

namespace cmk {

constexpr int SLICE_ROW = 6;         // a row of the per-pass table: (x0, y0, rx, ry, tw, th)

#pragma clang fp contract(off)

__device__ __forceinline__ float slice_clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(256) void slice_boxes_to_image_kernel(const float* __restrict__ det_box, const float* __restrict__ det_score,
                                                                  const int64_t* __restrict__ det_cls, const float* __restrict__ det_loc,
                                                                  const int32_t* __restrict__ det_counts, const float* __restrict__ table, int A,
                                                                  int K, float* __restrict__ cand_box, float* __restrict__ cand_score,
                                                                  int32_t* __restrict__ cand_cls, float* __restrict__ cand_loc,
                                                                  int32_t* __restrict__ cand_src, int32_t* __restrict__ cand_count) {
    const int a = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    int before = 0, total = 0;
    for (int i = 0; i < A; ++i) {
        const int c = min(max(det_counts[i], 0), K);
        if (i < a) before += c;
        total += c;
    }
    if (a == 0 && k == 0) cand_count[0] = total;
    if (k >= min(max(det_counts[a], 0), K)) return;          // rows at and beyond the count are never read
    const float* t = table + a * SLICE_ROW;
    const float x0 = t[0], y0 = t[1], rx = t[2], ry = t[3];
    const float xhi = x0 + t[4], yhi = y0 + t[5];            // the pass's own window in the image frame
    const long i = (long)a * K + k, o = (long)before + k;    // o < A * K: the sum of the clamped counts
    const float4 b = *reinterpret_cast<const float4*>(det_box + i * 4);
    float4 r;
    r.x = slice_clip(b.x * rx + x0, x0, xhi);
    r.y = slice_clip(b.y * ry + y0, y0, yhi);
    r.z = slice_clip(b.z * rx + x0, x0, xhi);
    r.w = slice_clip(b.w * ry + y0, y0, yhi);
    *reinterpret_cast<float4*>(cand_box + o * 4) = r;
    cand_score[o] = det_score[i];
    cand_cls[o] = (int32_t)det_cls[i];
    cand_loc[o * 2] = det_loc[i * 2] * rx + x0;
    cand_loc[o * 2 + 1] = det_loc[i * 2 + 1] * ry + y0;
    cand_src[o] = (int32_t)i;
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_slice_boxes_to_image(const float* det_box, const float* det_score, const int64_t* det_cls, const float* det_loc,
                                        const int32_t* det_counts, const float* table, int A, int K, int img_w, int img_h, float* cand_box,
                                        float* cand_score, int32_t* cand_cls, float* cand_loc, int32_t* cand_src, int32_t* cand_count,
                                        void* stream) {
    if (!det_box || !det_score || !det_cls || !det_loc || !det_counts || !table || !cand_box || !cand_score || !cand_cls || !cand_loc ||
        !cand_src || !cand_count)
        return fail(CMK_EINVAL, "slice_boxes_to_image: null pointer%s", "");
    if (A < 1 || A > 4096) return fail(CMK_EINVAL, "slice_boxes_to_image: need 1 <= A <= 4096 passes%s (A %ld, K %ld)", "", A, K);
    if (K < 1 || K > 65535) return fail(CMK_EINVAL, "slice_boxes_to_image: need 1 <= K <= 65535 rows%s (A %ld, K %ld)", "", A, K);
    if (img_w < 1 || img_h < 1 || img_w > 65535 || img_h > 65535)
        return fail(CMK_EINVAL, "slice_boxes_to_image: image size%s %ld x %ld outside [1, 65535]", "", img_h, img_w);
    if ((uintptr_t)det_box % 16 || (uintptr_t)cand_box % 16) return fail(CMK_EINVAL, "slice_boxes_to_image: boxes must be 16-byte aligned%s", "");
    hipLaunchKernelGGL(slice_boxes_to_image_kernel, dim3(cdiv(K, 256), A), dim3(256), 0, (hipStream_t)stream, det_box, det_score, det_cls, det_loc,
                       det_counts, table, A, K, cand_box, cand_score, cand_cls, cand_loc, cand_src, cand_count);
    return check_launch("slice_boxes_to_image");
}
