// The step in front of preprocess: detectron2's ResizeShortestEdge on a uint8 image, i.e. Pillow's 8-bit bilinear resampling
// (PIL.Image.resize(BILINEAR) -> Resample.c), reproduced byte for byte (deploy_utils.py:60-73 runs it on the CPU):
//   a horizontal pass (h, w, 3) -> (h, new_w, 3), rounded to uint8, then a vertical pass -> (new_h, new_w, 3); a pass whose input and
//   output length are equal is skipped.  Per output index the taps are [lo, lo + n) of the input with int32 weights k (scaled by 2^22;
//   the tables come from the host, include/cmk.h):  out = clamp((2^21 + sum pixel * k) >> 22, 0, 255).
// The vertical pass is fused with everything preprocess_kernel does (prepost.hip): it writes ((float)v - mean) / sd into the
// image's zero-padded slot of the NCHW batch, so the resized image never exists as floats outside the batch tensor.
// HBM-bound streaming kernels: the float stores (12 bytes per output pixel) dominate; the uint8 reads are a tenth of that.
#include "cmk_common.hpp"

#include <math.h>

namespace cmk {

constexpr int RESIZE_BITS = 22;      // Pillow's PRECISION_BITS for 8-bit bands: 32 - 8 - 2

__device__ __forceinline__ int resize_clip8(int acc) {
    acc >>= RESIZE_BITS;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// The tap range of output index i, clamped to the input so that a damaged table can never make a kernel read outside its source.
__device__ __forceinline__ void resize_bounds(const int32_t* __restrict__ bounds, int i, int ksize, int in_size, int& lo, int& n) {
    lo = bounds[2 * i];
    n = bounds[2 * i + 1];
    lo = lo < 0 ? 0 : (lo > in_size ? in_size : lo);
    n = n < 0 ? 0 : (n > ksize ? ksize : n);
    if (n > in_size - lo) n = in_size - lo;
}

// Horizontal pass.  The output (h, new_w, 3) is walked as a flat byte array, four consecutive bytes per thread and one aligned 32-bit
// store for them (dst comes 4-byte aligned); the last total % 4 bytes are stored one by one.  The three lanes of a pixel share their
// taps, and neighbouring lanes read neighbouring source bytes.
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int new_w,
                                                      const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize) {
    const long row = 3L * new_w, total = row * h;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q * 4 < total; q += (long)gridDim.x * 256) {
        const long e0 = q * 4;
        int y = (int)(e0 / row);
        int r = (int)(e0 - (long)y * row);
        int xx = r / 3, c = r - 3 * xx;
        uint32_t packed = 0;
        const int cnt = total - e0 < 4 ? (int)(total - e0) : 4;
        for (int j = 0; j < cnt; ++j) {
            int lo, n;
            resize_bounds(bounds, xx, ksize, w, lo, n);
            const uint8_t* p = src + ((long)y * w + lo) * 3 + c;
            const int32_t* k = kk + (long)xx * ksize;
            int acc = 1 << (RESIZE_BITS - 1);
            for (int t = 0; t < n; ++t) acc += (int)p[3 * t] * k[t];
            packed |= (uint32_t)resize_clip8(acc) << (8 * j);
            if (++c == 3) {
                c = 0;
                if (++xx == new_w) { xx = 0; ++y; }
            }
        }
        if (cnt == 4) *reinterpret_cast<uint32_t*>(dst + e0) = packed;
        else
            for (int j = 0; j < cnt; ++j) dst[e0 + j] = (uint8_t)(packed >> (8 * j));
    }
}

// One vertically resampled byte: column byte `off` of output row y of a source with `rowb` bytes per row and h rows.  kk == nullptr is
// the skipped pass (new_h == h): a copy.  lo / n / k are the same for a whole workgroup (one output row each).
__device__ __forceinline__ int resize_v_tap(const uint8_t* __restrict__ src, long rowb, long off, int lo, int n, const int32_t* __restrict__ k) {
    const uint8_t* p = src + lo * rowb + off;
    if (!k) return p[0];
    int acc = 1 << (RESIZE_BITS - 1);
    for (int t = 0; t < n; ++t) acc += (int)p[t * rowb] * k[t];
    return resize_clip8(acc);
}

// Vertical pass + normalise + pad.  grid = (ceil(W / 256), H): a thread owns output pixel (y, x) in all three planes, so a wave reads
// 192 consecutive source bytes per tap and each of its three float stores is 256 consecutive bytes of one channel plane.  FLIP: the
// thread reads the mirrored source column new_w - 1 - x instead (the wave's 192 bytes per tap run backwards, the stores stay as they are).
template <bool FLIP>
__device__ __forceinline__ void resize_v_preprocess_body(const uint8_t* __restrict__ src, float* __restrict__ dst, int h, int new_h, int new_w, int H,
                                                         int W, const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize, int reverse,
                                                         float m0, float m1, float m2, float s0, float s1, float s2) {
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const long plane = (long)H * W, o = (long)y * W + x;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;                  // zero padding on the right/bottom (applied after normalisation)
    if (y < new_h && x < new_w) {
        int lo = y, n = 1;
        const int32_t* k = nullptr;
        if (kk) {
            resize_bounds(bounds, y, ksize, h, lo, n);
            k = kk + (long)y * ksize;
        }
        const long rowb = 3L * new_w, sx = 3L * (FLIP ? new_w - 1 - x : x);
        const int a = resize_v_tap(src, rowb, sx, lo, n, k), b = resize_v_tap(src, rowb, sx + 1, lo, n, k),
                  c = resize_v_tap(src, rowb, sx + 2, lo, n, k);
        v0 = ((float)(reverse ? c : a) - m0) / s0;      // the expression of preprocess_kernel: the same bits
        v1 = ((float)b - m1) / s1;
        v2 = ((float)(reverse ? a : c) - m2) / s2;
    }
    dst[o] = v0;
    dst[plane + o] = v1;
    dst[2 * plane + o] = v2;
}

__global__ __launch_bounds__(256) void resize_v_preprocess_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int h, int new_h, int new_w,
                                                                 int H, int W, const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                                 int ksize, int reverse, float m0, float m1, float m2, float s0, float s1, float s2) {
    resize_v_preprocess_body<false>(src, dst, h, new_h, new_w, H, W, bounds, kk, ksize, reverse, m0, m1, m2, s0, s1, s2);
}

__global__ __launch_bounds__(256) void resize_v_preprocess_hflip_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int h, int new_h,
                                                                       int new_w, int H, int W, const int32_t* __restrict__ bounds,
                                                                       const int32_t* __restrict__ kk, int ksize, int reverse, float m0, float m1,
                                                                       float m2, float s0, float s1, float s2) {
    resize_v_preprocess_body<true>(src, dst, h, new_h, new_w, H, W, bounds, kk, ksize, reverse, m0, m1, m2, s0, s1, s2);
}

// Vertical pass alone, uint8 HWC out (the pure resize).  grid = (ceil(3 * new_w / 256), new_h): a thread per output byte.
__global__ __launch_bounds__(256) void resize_v_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int new_w,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk, int ksize) {
    const int y = blockIdx.y;
    const long rowb = 3L * new_w, off = (long)blockIdx.x * 256 + threadIdx.x;
    if (off >= rowb) return;
    int lo = y, n = 1;
    const int32_t* k = nullptr;
    if (kk) {
        resize_bounds(bounds, y, ksize, h, lo, n);
        k = kk + (long)y * ksize;
    }
    dst[y * rowb + off] = (uint8_t)resize_v_tap(src, rowb, off, lo, n, k);
}

// ---- test-time augmentation: the inverses of that geometry (include/cmk.h) -------------------------------------------------------
// A row of the per-augmentation table: (new_w, new_h, rx, ry, flip).
constexpr int TTA_ROW = 5;

// The tests restate this arithmetic in numpy, one rounded fp32 operation per step: nothing below may be fused into an fma.
#pragma clang fp contract(off)

// An x interval of an augmentation's frame mirrored inside [0, new_w]; every step is one rounded fp32 operation.
__device__ __forceinline__ void tta_flip_x(float nw, float& x0, float& x1) {
    const float a = nw - x1, b = nw - x0;
    x0 = a;
    x1 = b;
}

__device__ __forceinline__ float tta_clip(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }

// Detections of every augmentation -> one candidate set in the image frame.  grid = (ceil(K / 256), A): a thread owns detection k of
// augmentation a; its slot is k plus the counts of the augmentations before it (A uniform loads the scalar unit serves).
__global__ __launch_bounds__(256) void tta_boxes_to_image_kernel(const float* __restrict__ det_box, const float* __restrict__ det_score,
                                                                const int64_t* __restrict__ det_cls, const float* __restrict__ det_loc,
                                                                const int32_t* __restrict__ det_counts, const float* __restrict__ table, int A, int K,
                                                                float img_w, float img_h, float* __restrict__ cand_box, float* __restrict__ cand_score,
                                                                int32_t* __restrict__ cand_cls, float* __restrict__ cand_loc,
                                                                int32_t* __restrict__ cand_count) {
    const int a = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    int before = 0, total = 0;
    for (int i = 0; i < A; ++i) {
        const int c = min(max(det_counts[i], 0), K);
        if (i < a) before += c;
        total += c;
    }
    if (a == 0 && k == 0) cand_count[0] = total;
    if (k >= min(max(det_counts[a], 0), K)) return;
    const float* t = table + a * TTA_ROW;
    const float nw = t[0], rx = t[2], ry = t[3];
    const bool flip = t[4] != 0.f;
    const long i = (long)a * K + k, o = (long)before + k;
    const float4 b = *reinterpret_cast<const float4*>(det_box + i * 4);
    float x0 = b.x, x1 = b.z, lx = det_loc[i * 2];
    if (flip) {
        tta_flip_x(nw, x0, x1);
        lx = nw - lx;
    }
    float4 r;
    r.x = tta_clip(x0 * rx, img_w);
    r.y = tta_clip(b.y * ry, img_h);
    r.z = tta_clip(x1 * rx, img_w);
    r.w = tta_clip(b.w * ry, img_h);
    *reinterpret_cast<float4*>(cand_box + o * 4) = r;
    cand_score[o] = det_score[i];
    cand_cls[o] = (int32_t)det_cls[i];
    cand_loc[o * 2] = lx * rx;
    cand_loc[o * 2 + 1] = det_loc[i * 2 + 1] * ry;
}

// Merged boxes -> the frame of every augmentation.  grid = (ceil(K / 256), A): a thread owns row k of augmentation a.
__global__ __launch_bounds__(256) void tta_boxes_to_aug_kernel(const float* __restrict__ box, const int32_t* __restrict__ count,
                                                              const float* __restrict__ table, int A, int K, float* __restrict__ out_box,
                                                              int32_t* __restrict__ out_counts) {
    const int a = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int cnt = min(max(count[0], 0), K);
    if (k == 0) out_counts[a] = cnt;
    if (k >= K) return;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < cnt) {
        const float* t = table + a * TTA_ROW;
        const float nw = t[0], rx = t[2], ry = t[3];
        const float4 b = *reinterpret_cast<const float4*>(box + (long)k * 4);
        float x0 = b.x * rx, x1 = b.z * rx;
        if (t[4] != 0.f) tta_flip_x(nw, x0, x1);
        r = make_float4(x0, b.y * ry, x1, b.w * ry);
    }
    *reinterpret_cast<float4*>(out_box + ((long)a * K + k) * 4) = r;
}

// Mask average.  One thread per V consecutive output floats of a row (V = 4 where S % 4 == 0, else 1) with the loop over the
// augmentations inside, in order, starting from 0: a flipped augmentation's V floats are the V mirrored ones, read as one vector and
// reversed.  The threads after the K*S*S/V mask elements reduce the K mask scores.  Streaming: A reads per output float.
template <int V>
__global__ __launch_bounds__(256) void tta_reduce_masks_kernel(const float* __restrict__ masks, const int32_t* __restrict__ flips,
                                                              const float* __restrict__ mask_scores, const int32_t* __restrict__ count, int A,
                                                              int K, int S, float* __restrict__ out_masks, float* __restrict__ out_scores) {
    const int cnt = min(max(count[0], 0), K);
    const int rowv = S / V;                                  // vectors per row
    const long per = (long)S * rowv, nmask = (long)K * per, total = nmask + (out_scores ? K : 0);
    const float fa = (float)A;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
        if (q >= nmask) {
            const int k = (int)(q - nmask);
            float acc = 0.f;
            if (k < cnt) {
                for (int a = 0; a < A; ++a) acc = acc + mask_scores[(long)a * K + k];
                acc = acc / fa;
            }
            out_scores[k] = acc;
            continue;
        }
        const int k = (int)(q / per);
        const int r = (int)(q - (long)k * per);
        const int y = r / rowv, xv = r - y * rowv;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        if (k < cnt) {
            const long row = ((long)k * S + y) * S;
            const long img = (long)K * S * S;
            for (int a = 0; a < A; ++a) {
                const bool f = flips[a] != 0;
                const float* p = masks + a * img + row + (f ? S - V - xv * V : xv * V);
                float v[V];
                if constexpr (V == 4) {
                    const float4 t = *reinterpret_cast<const float4*>(p);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
                    v[0] = p[0];
                }
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = acc[j] + (f ? v[V - 1 - j] : v[j]);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = acc[j] / fa;
        }
        float* o = out_masks + q * V;
        if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else o[0] = acc[0];
    }
}

// Pillow's table width for one axis: ksize = int(ceil(max(in / out, 1))) * 2 + 1 (one IEEE division: nothing to contract).
inline int resize_ksize(int in_size, int out_size) {
    double scale = (double)in_size / (double)out_size;
    if (scale < 1.0) scale = 1.0;
    return (int)ceil(scale) * 2 + 1;
}

// A pass over an axis in -> out needs both tables and the ksize that belongs to the sizes; a skipped pass (in == out) takes no tables and ksize 0.
inline const char* resize_axis_error(int in_size, int out_size, const void* bounds, const void* kk, int ksize) {
    if (in_size == out_size && !bounds && !kk) return ksize == 0 ? nullptr : "ksize does not belong to these sizes";
    if (!bounds || !kk) return "null pointer";
    if (ksize != resize_ksize(in_size, out_size)) return "ksize does not belong to these sizes";
    return nullptr;
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_resize_ksize(int in_size, int out_size) {
    if (in_size < 1 || out_size < 1) return 0;
    return resize_ksize(in_size, out_size);
}

extern "C" int cmk_resize_h_u8(const uint8_t* src, int h, int w, int new_w, const int32_t* bounds_x, const int32_t* kk_x, int ksize_x,
                               uint8_t* dst, void* stream) {
    if (!src || !dst || !bounds_x || !kk_x) return fail(CMK_EINVAL, "resize_h: null pointer%s", "");
    if (h < 1 || w < 1 || new_w < 1) return fail(CMK_EINVAL, "resize_h: empty image%s (h %ld, w %ld)", "", h, w);
    if (ksize_x != resize_ksize(w, new_w))
        return fail(CMK_EINVAL, "resize_h: ksize%s %ld does not belong to these sizes (expected %ld)", "", ksize_x, resize_ksize(w, new_w));
    if ((uintptr_t)dst % 4) return fail(CMK_EINVAL, "resize_h: dst must be 4-byte aligned%s", "");
    const long quads = (3L * new_w * h + 3) / 4;
    long grid = (quads + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(resize_h_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, src, dst, h, w, new_w, bounds_x, kk_x, ksize_x);
    return check_launch("resize_h");
}

extern "C" int cmk_resize_v_u8(const uint8_t* src, int h, int new_h, int new_w, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                               uint8_t* dst, void* stream) {
    if (!src || !dst) return fail(CMK_EINVAL, "resize_v: null pointer%s", "");
    if (h < 1 || new_h < 1 || new_w < 1) return fail(CMK_EINVAL, "resize_v: empty image%s (h %ld, new_h %ld)", "", h, new_h);
    if (new_h > 65535) return fail(CMK_EINVAL, "resize_v: more than 65535 output rows%s", "");
    if (const char* e = resize_axis_error(h, new_h, bounds_y, kk_y, ksize_y)) return fail(CMK_EINVAL, "resize_v: %s (h %ld, new_h %ld)", e, h, new_h);
    hipLaunchKernelGGL(resize_v_u8_kernel, dim3((int)((3L * new_w + 255) / 256), new_h), dim3(256), 0, (hipStream_t)stream, src, dst, h, new_w,
                       bounds_y, kk_y, ksize_y);
    return check_launch("resize_v");
}

extern "C" int cmk_resize_v_preprocess(const uint8_t* src, int h, int new_h, int new_w, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                                       float* dst, int H, int W, const float* mean3, const float* std3, int reverse_channels, void* stream) {
    if (!src || !dst || !mean3 || !std3) return fail(CMK_EINVAL, "resize_v_preprocess: null pointer%s", "");
    if (h < 1 || new_h < 1 || new_w < 1) return fail(CMK_EINVAL, "resize_v_preprocess: empty image%s (h %ld, new_h %ld)", "", h, new_h);
    if (H < new_h || W < new_w) return fail(CMK_EINVAL, "resize_v_preprocess: padded size smaller than the resized image%s", "");
    if (H > 65535) return fail(CMK_EINVAL, "resize_v_preprocess: more than 65535 rows%s", "");
    if (const char* e = resize_axis_error(h, new_h, bounds_y, kk_y, ksize_y))
        return fail(CMK_EINVAL, "resize_v_preprocess: %s (h %ld, new_h %ld)", e, h, new_h);
    hipLaunchKernelGGL(resize_v_preprocess_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, src, dst, h, new_h, new_w, H, W,
                       bounds_y, kk_y, ksize_y, reverse_channels ? 1 : 0, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return check_launch("resize_v_preprocess");
}

extern "C" int cmk_resize_v_preprocess_hflip(const uint8_t* src, int h, int new_h, int new_w, const int32_t* bounds_y, const int32_t* kk_y,
                                             int ksize_y, float* dst, int H, int W, const float* mean3, const float* std3, int reverse_channels,
                                             void* stream) {
    if (!src || !dst || !mean3 || !std3) return fail(CMK_EINVAL, "resize_v_preprocess_hflip: null pointer%s", "");
    if (h < 1 || new_h < 1 || new_w < 1) return fail(CMK_EINVAL, "resize_v_preprocess_hflip: empty image%s (h %ld, new_h %ld)", "", h, new_h);
    if (H < new_h || W < new_w) return fail(CMK_EINVAL, "resize_v_preprocess_hflip: padded size smaller than the resized image%s", "");
    if (H > 65535) return fail(CMK_EINVAL, "resize_v_preprocess_hflip: more than 65535 rows%s", "");
    if (const char* e = resize_axis_error(h, new_h, bounds_y, kk_y, ksize_y))
        return fail(CMK_EINVAL, "resize_v_preprocess_hflip: %s (h %ld, new_h %ld)", e, h, new_h);
    hipLaunchKernelGGL(resize_v_preprocess_hflip_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, src, dst, h, new_h, new_w, H, W,
                       bounds_y, kk_y, ksize_y, reverse_channels ? 1 : 0, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return check_launch("resize_v_preprocess_hflip");
}

// The limits the TTA kernels index with: A rides in gridDim.y, A * K * S * S stays far below 2^63 and K * S * S / V below 2^31 * 4096.
static const char* tta_dims_error(int A, int K) {
    if (A < 1 || A > 4096) return "need 1 <= A <= 4096 augmentations";
    if (K < 1 || K > 65535) return "need 1 <= K <= 65535 rows";
    return nullptr;
}

extern "C" int cmk_tta_boxes_to_image(const float* det_box, const float* det_score, const int64_t* det_cls, const float* det_loc,
                                      const int32_t* det_counts, const float* table, int A, int K, int img_w, int img_h, float* cand_box,
                                      float* cand_score, int32_t* cand_cls, float* cand_loc, int32_t* cand_count, void* stream) {
    if (!det_box || !det_score || !det_cls || !det_loc || !det_counts || !table || !cand_box || !cand_score || !cand_cls || !cand_loc || !cand_count)
        return fail(CMK_EINVAL, "tta_boxes_to_image: null pointer%s", "");
    if (const char* e = tta_dims_error(A, K)) return fail(CMK_EINVAL, "tta_boxes_to_image: %s (A %ld, K %ld)", e, A, K);
    if (img_w < 1 || img_h < 1 || img_w > 65535 || img_h > 65535)
        return fail(CMK_EINVAL, "tta_boxes_to_image: image size%s %ld x %ld outside [1, 65535]", "", img_h, img_w);
    if ((uintptr_t)det_box % 16 || (uintptr_t)cand_box % 16) return fail(CMK_EINVAL, "tta_boxes_to_image: boxes must be 16-byte aligned%s", "");
    hipLaunchKernelGGL(tta_boxes_to_image_kernel, dim3(cdiv(K, 256), A), dim3(256), 0, (hipStream_t)stream, det_box, det_score, det_cls, det_loc,
                       det_counts, table, A, K, (float)img_w, (float)img_h, cand_box, cand_score, cand_cls, cand_loc, cand_count);
    return check_launch("tta_boxes_to_image");
}

extern "C" int cmk_tta_boxes_to_aug(const float* box, const int32_t* count, const float* table, int A, int K, float* out_box, int32_t* out_counts,
                                    void* stream) {
    if (!box || !count || !table || !out_box || !out_counts) return fail(CMK_EINVAL, "tta_boxes_to_aug: null pointer%s", "");
    if (const char* e = tta_dims_error(A, K)) return fail(CMK_EINVAL, "tta_boxes_to_aug: %s (A %ld, K %ld)", e, A, K);
    if ((uintptr_t)box % 16 || (uintptr_t)out_box % 16) return fail(CMK_EINVAL, "tta_boxes_to_aug: boxes must be 16-byte aligned%s", "");
    hipLaunchKernelGGL(tta_boxes_to_aug_kernel, dim3(cdiv(K, 256), A), dim3(256), 0, (hipStream_t)stream, box, count, table, A, K, out_box, out_counts);
    return check_launch("tta_boxes_to_aug");
}

extern "C" int cmk_tta_reduce_masks(const float* masks, const int32_t* flips, const float* mask_scores, const int32_t* count, int A, int K, int S,
                                    float* out_masks, float* out_scores, void* stream) {
    if (!masks || !flips || !count || !out_masks) return fail(CMK_EINVAL, "tta_reduce_masks: null pointer%s", "");
    if (!mask_scores != !out_scores) return fail(CMK_EINVAL, "tta_reduce_masks: null pointer%s (mask_scores and out_scores go together)", "");
    if (const char* e = tta_dims_error(A, K)) return fail(CMK_EINVAL, "tta_reduce_masks: %s (A %ld, K %ld)", e, A, K);
    if (S < 1 || S > 1024) return fail(CMK_EINVAL, "tta_reduce_masks: need 1 <= S <= 1024%s, got %ld", "", S);
    const bool vec = S % 4 == 0 && (uintptr_t)masks % 16 == 0 && (uintptr_t)out_masks % 16 == 0;
    const long work = (long)K * S * (S / (vec ? 4 : 1)) + (out_scores ? K : 0);
    if (vec)
        hipLaunchKernelGGL(tta_reduce_masks_kernel<4>, dim3(stream_grid(work)), dim3(256), 0, (hipStream_t)stream, masks, flips, mask_scores, count, A, K,
                           S, out_masks, out_scores);
    else
        hipLaunchKernelGGL(tta_reduce_masks_kernel<1>, dim3(stream_grid(work)), dim3(256), 0, (hipStream_t)stream, masks, flips, mask_scores, count, A, K,
                           S, out_masks, out_scores);
    return check_launch("tta_reduce_masks");
}
