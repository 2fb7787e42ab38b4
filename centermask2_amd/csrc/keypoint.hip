// Keypoint heatmap decode of the keypoint R-CNN head (KRCNNConvDeconvUpsampleHead, MODEL.KEYPOINT_ON): from the packed score_lowres
// output to (x, y, score) per (RoI, keypoint), i.e. the tail of keypoint_head.py:219-224 (bilinear x2) and keypoint_rcnn_inference
// keypoint_head.py:89-116 -> detectron2 heatmaps_to_keypoints (source absent; its published behaviour is restated here).
//
// Per RoI with box (x0, y0, x1, y1): w = max(x1-x0, 1), h = max(y1-y0, 1), Wc = ceil(w), Hc = ceil(h).  Per keypoint k:
//   map28 = depth-to-space of the packed deconv: map28[2a+py][2b+px] = dec[a][b][(2py+px)*K + k]          (2S x 2S)
//   map56 = upsample_bilinear2d(map28, x2, align_corners=False)                                            (4S x 4S, in LDS)
//   roi   = upsample_bicubic2d(map56, (Hc, Wc), align_corners=False), evaluated on the fly, never stored
//   m     = max(roi), (yi, xi) = its FIRST position in row-major order
//   score = exp(roi[yi][xi] - m) / sum(exp(map56 - m)) = 1 / sum(exp(map56 - m))
//   x = (xi + 0.5) * (w / Wc) + x0,  y = (yi + 0.5) * (h / Hc) + y0
// The launch is static (so that it can be captured in a graph with the RoI heads): KP_SPLIT workgroups per (RoI, keypoint) each
// take a contiguous band of the Hc rows (one band per KP_BAND_PIXELS output pixels, at most KP_SPLIT), write their (max, first
// argmax) to the workspace, and a second launch combines the bands in row order.  Every reduction runs in a fixed order and a tie
// goes to the lower row-major index, so the result does not depend on the tiling or on timing.  No atomics.
#include <math.h>

#include "cmk_common.hpp"

namespace cmk {

constexpr int KP_SPLIT = 8;             // workgroups (row bands) per (RoI, keypoint) at most
constexpr int KP_BAND_PIXELS = 8192;    // a box gets one band per this many output pixels
constexpr int KP_MAX_S = 16;            // deconv input resolution S: map56 is at most 64 x 64 floats of LDS
constexpr int KP_THREADS = 256;
constexpr int KP_ROWS = 8;             // output rows per step of a band (one vertical pass, then the column weights serve them all)
static_assert(KP_THREADS == 256, "the block reductions combine exactly four waves");
// workspace record per (RoI, keypoint): KP_SPLIT band records {max, row, col, -}, then {max of map56, sum exp(map56 - that max), -, -}
constexpr int KP_WS_WORDS = 4 * (KP_SPLIT + 1);

struct KpBox {
    float x0, y0, w, h;
    int wc, hc;
};

__device__ inline KpBox kp_box(const float* b) {
    KpBox r;
    r.x0 = b[0];
    r.y0 = b[1];
    r.w = fmaxf(__fsub_rn(b[2], b[0]), 1.0f);          // widths.clamp(min=1)
    r.h = fmaxf(__fsub_rn(b[3], b[1]), 1.0f);
    r.wc = (int)ceilf(r.w);
    r.hc = (int)ceilf(r.h);
    return r;
}

// PyTorch's cubic convolution weights (A = -0.75) of the four taps around the fractional position t in [0, 1)
__device__ inline void cubic_coeffs(float t, float c[4]) {
    const float A = -0.75f;
    const float x1 = t + 1.0f, x2 = 1.0f - t, x3 = x2 + 1.0f;
    c[0] = ((A * x1 - 5.0f * A) * x1 + 8.0f * A) * x1 - 4.0f * A;
    c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

// bicubic source position of output index d: scale * (d + 0.5) - 0.5, NOT clamped; returns its floor, t = the remainder
__device__ inline int cubic_src(float scale, int d, float& t) {
    const float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f);
    const float f = floorf(s);
    t = __fsub_rn(s, f);
    return (int)f;
}

// (v1, y1, x1) wins over (v2, y2, x2): a larger value, or the same value earlier in row-major order.  As in torch.max / argmax a NaN
// counts as larger than every number, and the first NaN wins.
__device__ inline bool kp_better(float v1, int y1, int x1, float v2, int y2, int x2) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 != n2) return n1;
    if (!n1 && v1 != v2) return v1 > v2;
    return y1 < y2 || (y1 == y2 && x1 < x2);
}

// map56 = bilinear x2 of the depth-to-space map of keypoint k of RoI r, built in LDS; returns its side 4S
__device__ inline int kp_build_map(const float* __restrict__ dec, int cs, int co, int S, int K, long r, int k, float* m28, float* m56) {
    const int S2 = 2 * S, S4 = 4 * S;
    const float* base = dec + r * S * S * cs + co + k;
    for (int i = threadIdx.x; i < S2 * S2; i += KP_THREADS) {
        const int y = i / S2, x = i - y * S2;
        m28[i] = base[((long)(y >> 1) * S + (x >> 1)) * cs + ((y & 1) * 2 + (x & 1)) * K];
    }
    __syncthreads();
    // upsample_bilinear2d, align_corners=False, scale 1/2: src = 0.5 * (dst + 0.5) - 0.5 clamped at 0, upper tap min(i + 1, 2S - 1)
    for (int i = threadIdx.x; i < S4 * S4; i += KP_THREADS) {
        const int oy = i / S4, ox = i - oy * S4;
        const float sy = fmaxf(__fsub_rn(__fmul_rn(0.5f, __fadd_rn((float)oy, 0.5f)), 0.5f), 0.0f);
        const float sx = fmaxf(__fsub_rn(__fmul_rn(0.5f, __fadd_rn((float)ox, 0.5f)), 0.5f), 0.0f);
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < S2 - 1 ? 1 : 0), x1 = x0 + (x0 < S2 - 1 ? 1 : 0);
        const float ly1 = sy - (float)y0, lx1 = sx - (float)x0;
        const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
        m56[i] = ly0 * (lx0 * m28[y0 * S2 + x0] + lx1 * m28[y0 * S2 + x1]) + ly1 * (lx0 * m28[y1 * S2 + x0] + lx1 * m28[y1 * S2 + x1]);
    }
    __syncthreads();
    return S4;
}

// block-wide (value, row, col) arg-max in a fixed order; the result is valid in every thread
__device__ inline void kp_block_argmax(float& v, int& y, int& x, float* red_v, int* red_y, int* red_x) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int y2 = __shfl_xor(y, o, 64), x2 = __shfl_xor(x, o, 64);
        if (kp_better(v2, y2, x2, v, y, x)) { v = v2; y = y2; x = x2; }
    }
    __syncthreads();
    if (lane == 0) { red_v[wave] = v; red_y[wave] = y; red_x[wave] = x; }
    __syncthreads();
    v = red_v[0]; y = red_y[0]; x = red_x[0];
    for (int w = 1; w < KP_THREADS / 64; ++w)
        if (kp_better(red_v[w], red_y[w], red_x[w], v, y, x)) { v = red_v[w]; y = red_y[w]; x = red_x[w]; }
}

// Stage 1.  grid = R * K * KP_SPLIT workgroups; workgroup `band` of (r, k) evaluates rows [band * rows, (band + 1) * rows) of the
// Hc x Wc bicubic map.  Band 0 also leaves the exp-sum of map56 behind.
__global__ __launch_bounds__(KP_THREADS) void keypoint_band_kernel(const float* __restrict__ dec, int cs, int co, int S, int K,
                                                                   const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                                   int topk, float* __restrict__ ws) {
    __shared__ float m28[4 * KP_MAX_S * KP_MAX_S];
    __shared__ float m56[16 * KP_MAX_S * KP_MAX_S];
    __shared__ float tmp[2 * KP_ROWS * 4 * KP_MAX_S];
    __shared__ float red_v[KP_THREADS / 64];
    __shared__ int red_y[KP_THREADS / 64], red_x[KP_THREADS / 64];
    const int band = blockIdx.x % KP_SPLIT;
    const long rk = blockIdx.x / KP_SPLIT;
    const int k = (int)(rk % K);
    const long r = rk / K;
    const int n = (int)(r / topk), slot = (int)(r - (long)n * topk);
    if (slot >= counts[n]) return;                         // stage 2 writes the zeros
    const KpBox bx = kp_box(boxes + r * 4);
    const long pixels = (long)bx.hc * bx.wc;
    const int nbands = (int)min((long)KP_SPLIT, max(1L, (pixels + KP_BAND_PIXELS - 1) / KP_BAND_PIXELS));
    const int rows = cdiv(bx.hc, nbands);
    const int row0 = band * rows, row1 = min(bx.hc, row0 + rows);
    float* rec = ws + rk * KP_WS_WORDS;
    int* irec = reinterpret_cast<int*>(rec);
    if (band >= nbands || row0 >= row1) {                  // no rows in this band: an empty record
        if (threadIdx.x == 0) {
            rec[band * 4] = -INFINITY;
            irec[band * 4 + 1] = -1;
            irec[band * 4 + 2] = -1;
        }
        return;
    }
    const int S4 = kp_build_map(dec, cs, co, S, K, r, k, m28, m56);
    if (band == 0) {                                       // sum(exp(map56 - max(map56))); stage 2 rescales it to the final max
        float mx = -INFINITY;
        for (int i = threadIdx.x; i < S4 * S4; i += KP_THREADS) mx = fmaxf(mx, m56[i]);
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0) red_v[threadIdx.x >> 6] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red_v[0], red_v[1]), fmaxf(red_v[2], red_v[3]));
        float sum = 0.f;
        for (int i = threadIdx.x; i < S4 * S4; i += KP_THREADS) sum += expf(m56[i] - mx);
        sum = wave_sum(sum);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red_v[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            rec[KP_SPLIT * 4] = mx;
            rec[KP_SPLIT * 4 + 1] = (red_v[0] + red_v[1]) + (red_v[2] + red_v[3]);
        }
    }
    // upsample_bicubic2d to (Hc, Wc), align_corners=False: scale = 4S / out in fp32, taps clamped to [0, 4S - 1].  The two axes are
    // separable: per group of KP_ROWS output rows the vertical pass runs once into LDS (4S values per row), then every thread computes its
    // columns' weights once and applies them to all rows of the group.  tmp is double-buffered: one barrier per group.
    const float scale_y = (float)S4 / (float)bx.hc, scale_x = (float)S4 / (float)bx.wc;
    const int wc = bx.wc;
    float best = -INFINITY;
    int by = 0x7fffffff, bxi = 0x7fffffff;
    int buf = 0;
    for (int g0 = row0; g0 < row1; g0 += KP_ROWS, buf ^= 1) {
        const int nr = min(KP_ROWS, row1 - g0);
        float* t = tmp + buf * (KP_ROWS * 4 * KP_MAX_S);
        for (int i = threadIdx.x; i < nr * S4; i += KP_THREADS) {
            const int g = i / S4, c = i - g * S4;
            float ty, cy[4];
            const int iy = cubic_src(scale_y, g0 + g, ty);
            cubic_coeffs(ty, cy);
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) v += m56[min(max(iy - 1 + j, 0), S4 - 1) * S4 + c] * cy[j];
            t[g * S4 + c] = v;
        }
        __syncthreads();
        for (int ox = threadIdx.x; ox < wc; ox += KP_THREADS) {
            float tx, cx[4];
            const int ix = cubic_src(scale_x, ox, tx);
            cubic_coeffs(tx, cx);
            int xs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) xs[j] = min(max(ix - 1 + j, 0), S4 - 1);
            for (int g = 0; g < nr; ++g) {
                const float* row = t + g * S4;
                const float v = ((row[xs[0]] * cx[0] + row[xs[1]] * cx[1]) + row[xs[2]] * cx[2]) + row[xs[3]] * cx[3];
                if (kp_better(v, g0 + g, ox, best, by, bxi)) { best = v; by = g0 + g; bxi = ox; }
            }
        }
    }
    kp_block_argmax(best, by, bxi, red_v, red_y, red_x);
    if (threadIdx.x == 0) {
        rec[band * 4] = best;
        irec[band * 4 + 1] = by;
        irec[band * 4 + 2] = bxi;
    }
}

// Stage 2.  One thread per (RoI, keypoint): combine the bands in row order and write (x, y, score); rows past counts get zeros.
__global__ __launch_bounds__(KP_THREADS) void keypoint_finish_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                                     int topk, int K, long RK, const float* __restrict__ ws,
                                                                     float* __restrict__ out) {
    const long i = (long)blockIdx.x * KP_THREADS + threadIdx.x;
    if (i >= RK) return;
    const long r = i / K;
    const int n = (int)(r / topk), slot = (int)(r - (long)n * topk);
    float* o = out + i * 3;
    if (slot >= counts[n]) {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
        return;
    }
    const float* rec = ws + i * KP_WS_WORDS;
    const int* irec = reinterpret_cast<const int*>(rec);
    float v = rec[0];
    int y = irec[1], x = irec[2];
    for (int b = 1; b < KP_SPLIT; ++b) {
        if (irec[b * 4 + 1] < 0) break;                    // the bands past the box's last row are empty
        if (kp_better(rec[b * 4], irec[b * 4 + 1], irec[b * 4 + 2], v, y, x)) { v = rec[b * 4]; y = irec[b * 4 + 1]; x = irec[b * 4 + 2]; }
    }
    const KpBox bx = kp_box(boxes + r * 4);
    const float total = rec[KP_SPLIT * 4 + 1] * expf(rec[KP_SPLIT * 4] - v);     // sum(exp(map56 - m))
    o[0] = __fadd_rn(__fmul_rn(__fadd_rn((float)x, 0.5f), __fdiv_rn(bx.w, (float)bx.wc)), bx.x0);
    o[1] = __fadd_rn(__fmul_rn(__fadd_rn((float)y, 0.5f), __fdiv_rn(bx.h, (float)bx.hc)), bx.y0);
    o[2] = 1.0f / total;
}

}  // namespace cmk

using namespace cmk;

extern "C" int64_t cmk_keypoint_decode_ws_len(int R, int K) {
    if (R < 1 || K < 1) return 0;
    return (int64_t)R * K * KP_WS_WORDS;
}

extern "C" int cmk_keypoint_decode(const float* dec, int dec_cs, int dec_co, int S, int K, const float* boxes, const int32_t* counts, int N,
                                   int topk, float* ws, int64_t ws_len, float* out, void* stream) {
    if (!dec || !boxes || !counts || !ws || !out) return fail(CMK_EINVAL, "keypoint_decode: null pointer%s", "");
    if (K < 1) return fail(CMK_EINVAL, "keypoint_decode: %sK = %ld keypoints, need at least 1", "", (long)K);
    if (S < 1 || S > KP_MAX_S) return fail(CMK_EINVAL, "keypoint_decode: %sresolution %ld outside [1, %ld]", "", (long)S, (long)KP_MAX_S);
    if (N < 1 || topk < 1 || dec_co < 0 || (long)dec_cs < (long)dec_co + 4L * K) return fail(CMK_EINVAL, "keypoint_decode: bad shape%s", "");
    const long R = (long)N * topk;
    if (R * K * KP_SPLIT * KP_THREADS > 0xffffffffL)          // the launch's work-item count must fit in 32 bits
        return fail(CMK_EINVAL, "keypoint_decode: %s%ld RoIs x keypoints is too many", "", R * K);
    if (ws_len < R * K * KP_WS_WORDS) return fail(CMK_EINVAL, "keypoint_decode: %sworkspace of %ld words, need %ld", "", (long)ws_len, R * K * KP_WS_WORDS);
    hipLaunchKernelGGL(keypoint_band_kernel, dim3((unsigned)(R * K * KP_SPLIT)), dim3(KP_THREADS), 0, (hipStream_t)stream, dec, dec_cs, dec_co,
                       S, K, boxes, counts, topk, ws);
    const int rc = check_launch("keypoint_decode (bands)");
    if (rc) return rc;
    hipLaunchKernelGGL(keypoint_finish_kernel, dim3((unsigned)((R * K + KP_THREADS - 1) / KP_THREADS)), dim3(KP_THREADS), 0,
                       (hipStream_t)stream, boxes, counts, topk, K, R * K, ws, out);
    return check_launch("keypoint_decode (finish)");
}
