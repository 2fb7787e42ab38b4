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
// 192 consecutive source bytes per tap and each of its three float stores is 256 consecutive bytes of one channel plane.
__global__ __launch_bounds__(256) void resize_v_preprocess_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int h, int new_h, int new_w,
                                                                 int H, int W, const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                                 int ksize, int reverse, float m0, float m1, float m2, float s0, float s1, float s2) {
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
        const long rowb = 3L * new_w;
        const int a = resize_v_tap(src, rowb, 3L * x, lo, n, k), b = resize_v_tap(src, rowb, 3L * x + 1, lo, n, k),
                  c = resize_v_tap(src, rowb, 3L * x + 2, lo, n, k);
        v0 = ((float)(reverse ? c : a) - m0) / s0;      // the expression of preprocess_kernel: the same bits
        v1 = ((float)b - m1) / s1;
        v2 = ((float)(reverse ? a : c) - m2) / s2;
    }
    dst[o] = v0;
    dst[plane + o] = v1;
    dst[2 * plane + o] = v2;
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
