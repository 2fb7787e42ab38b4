// Depth-wise 3x3 of an inverted-residual block (MobileNetV2: mobilenet.py:38-76) with everything around it that is per-element:
//   y = clamp(dw3x3(min(x, in_max)) * scale[c] + shift[c], out_min, out_max)           pad 1, stride 1 | 2, NHWC channel-slice views.
// min(x, in_max) is the upper half of the ReLU6 of the PRODUCER (the stem or the expand 1x1, which run on the ordinary conv kernels with
// their plain ReLU epilogue and are read by nobody else): min(relu(v), 6) == relu6(v) bit for bit.  scale/shift is the folded FrozenBN of
// the depth-wise conv, [out_min, out_max] = [0, 6] its own ReLU6.  The zero padding stands for zeros of the clamped input, so the
// border taps are skipped, never replaced by `shift`.  Infinite bounds switch a clamp off.  Both clamps are written as selects: a NaN
// fails every comparison and passes through, as in torch.nn.ReLU6 (fminf / fmaxf would return the bound instead).
// PLAIN is the bare depth-wise 3x3 (vovnet.py:110-119 'dw_conv3x3': no bias, no activation; the point-wise 1x1 + FrozenBN + ReLU that
// follows is an ordinary conv launch): y = dw3x3(x), both clamps and the affine compiled out, scale / shift never read.
//
// HBM-bound (1 FMA per 4 bytes at best): one thread = 4 channels x T adjacent output columns x R output rows, 16-byte loads and stores,
// the ((R-1)*S+3) x ((T-1)*S+3) input quads each loaded once per thread, the 9 weight quads and the affine in registers.  Rows matter more
// than columns: horizontally adjacent windows belong to neighbouring lanes and meet in the L1, vertically adjacent ones belong to other
// workgroups and meet in the L2, which R = 4 reads 1.5x instead of 3x (stride 1).  The tile is chosen on the host so that the small maps
// (25x40 at batch 8) still give every CU several workgroups.
#include <math.h>

#include "cmk_common.hpp"

namespace cmk {

typedef float dwq __attribute__((ext_vector_type(4)));

__device__ inline float clamp_hi(float v, float hi) { return v > hi ? hi : v; }                     // NaN stays NaN
__device__ inline float clamp_lo_hi(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int S, int T, int R, bool PLAIN>
__global__ __launch_bounds__(256) void dwconv3_bn_act_kernel(const float* __restrict__ x, int x_cs, int x_co, const float* __restrict__ w,
                                                            const float* __restrict__ scale, const float* __restrict__ shift, float in_max,
                                                            float out_min, float out_max, float* __restrict__ y, int y_cs, int y_co, int N,
                                                            int H, int W, int Ho, int Wo, int C4) {
    const int WT = (Wo + T - 1) / T, HT = (Ho + R - 1) / R;
    const int total = N * HT * WT * C4;               // <= 2^31 - DW_MAX_GRID_STRIDE, checked on the host: i never wraps
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int c4 = i % C4;
        int r = i / C4;
        const int wt = r % WT;
        r /= WT;
        const int ht = r % HT;
        const int n = r / HT;
        dwq wq[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wq[t] = *reinterpret_cast<const dwq*>(w + (long)t * C4 * 4 + c4 * 4);
        dwq acc[R][T];
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int j = 0; j < T; ++j) acc[q][j] = dwq{0.f, 0.f, 0.f, 0.f};
        const int oh0 = ht * R, iw0 = wt * T * S - 1;
        constexpr int COLS = (T - 1) * S + 3, ROWS = (R - 1) * S + 3;
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int ih = oh0 * S - 1 + rr;
            if (ih < 0 || ih >= H) continue;
            const float* row = x + ((long)n * H + ih) * W * x_cs + x_co + c4 * 4;
#pragma unroll
            for (int cc = 0; cc < COLS; ++cc) {
                const int iw = iw0 + cc;
                dwq v = {0.f, 0.f, 0.f, 0.f};
                if (iw >= 0 && iw < W) {
                    v = *reinterpret_cast<const dwq*>(row + (long)iw * x_cs);
                    if (!PLAIN) { v.x = clamp_hi(v.x, in_max); v.y = clamp_hi(v.y, in_max); v.z = clamp_hi(v.z, in_max); v.w = clamp_hi(v.w, in_max); }
                }
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const int kh = rr - q * S;           // compile-time after unrolling, like kw
                    if (kh < 0 || kh >= 3) continue;
#pragma unroll
                    for (int j = 0; j < T; ++j) {
                        const int kw = cc - j * S;
                        if (kw >= 0 && kw < 3) {
                            const dwq wv = wq[kh * 3 + kw];
                            acc[q][j].x = fmaf(v.x, wv.x, acc[q][j].x); acc[q][j].y = fmaf(v.y, wv.y, acc[q][j].y);
                            acc[q][j].z = fmaf(v.z, wv.z, acc[q][j].z); acc[q][j].w = fmaf(v.w, wv.w, acc[q][j].w);
                        }
                    }
                }
            }
        }
        dwq sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
        if (!PLAIN) {
            sc = *reinterpret_cast<const dwq*>(scale + c4 * 4);
            sh = *reinterpret_cast<const dwq*>(shift + c4 * 4);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int oh = oh0 + q;
            if (oh >= Ho) continue;
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const int ow = wt * T + j;
                if (ow < Wo) {
                    dwq o = acc[q][j];
                    if (!PLAIN) {
                        o.x = clamp_lo_hi(fmaf(o.x, sc.x, sh.x), out_min, out_max);
                        o.y = clamp_lo_hi(fmaf(o.y, sc.y, sh.y), out_min, out_max);
                        o.z = clamp_lo_hi(fmaf(o.z, sc.z, sh.z), out_min, out_max);
                        o.w = clamp_lo_hi(fmaf(o.w, sc.w, sh.w), out_min, out_max);
                    }
                    *reinterpret_cast<dwq*>(y + (((long)n * Ho + oh) * Wo + ow) * y_cs + y_co + c4 * 4) = o;
                }
            }
        }
    }
}

struct DwArgs {
    const float *x, *w, *scale, *shift;
    float* y;
    int x_cs, x_co, y_cs, y_co, N, H, W, Ho, Wo, C4;
    float in_max, out_min, out_max;
    void* stream;
};

// The kernel walks its threads with a 32-bit index and a grid stride of at most 8192 workgroups x 256 (launch_dw).  The entry points
// refuse an output of more than 2^31 - DW_MAX_GRID_STRIDE quads (a thread owns at least one), so the index that ends the loop,
// below total + stride, stays below 2^31.  A bound, not a 64-bit index: the kernel and its registers stay as they are.
constexpr long DW_MAX_GRID_STRIDE = 8192L * 256;

// what both entry points ask of their views and shape after the null and empty-shape checks; nullptr or the reason of the refusal
static const char* dw_view_error(const float* x, int x_cs, int x_co, const float* y, int y_cs, int y_co, int C) {
    if (C & 3) return "C must be a multiple of 4";
    if ((x_cs & 3) || (x_co & 3) || (y_cs & 3) || (y_co & 3) || x_co < 0 || y_co < 0)
        return "misaligned channel offset or pixel stride (multiples of 4 floats, offsets >= 0)";
    if ((long)x_co + C > x_cs || (long)y_co + C > y_cs) return "channel slice [co, co + C) leaves the pixel";
    return nullptr;
}

// x == y is fine for disjoint channel slices; overlapping ones are refused: a thread would read what another has written
static bool dw_overlap(const float* x, int x_co, const float* y, int y_co, int C) { return x == y && x_co < y_co + C && y_co < x_co + C; }

static inline long dw_blocks(const DwArgs& a, int t, int r) {
    return ((long)a.N * ((a.Ho + r - 1) / r) * ((a.Wo + t - 1) / t) * a.C4 + 255) / 256;
}

template <int S, int T, int R, bool PLAIN = false>
static void launch_dw(const DwArgs& a) {
    const long blocks = dw_blocks(a, T, R);
    const unsigned grid = PLAIN ? (unsigned)stream_grid(blocks * 256) : (unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));
    hipLaunchKernelGGL((dwconv3_bn_act_kernel<S, T, R, PLAIN>), dim3(grid), dim3(256), 0, (hipStream_t)a.stream, a.x, a.x_cs, a.x_co, a.w, a.scale, a.shift,
                       a.in_max, a.out_min, a.out_max, a.y, a.y_cs, a.y_co, a.N, a.H, a.W, a.Ho, a.Wo, a.C4);
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_dwconv3x3_bn_act_nhwc(const float* x, int x_cs, int x_co, const float* w, const float* scale, const float* shift,
                                         float in_max, float out_min, float out_max, float* y, int y_cs, int y_co, int N, int H, int W, int C,
                                         int stride, void* stream) {
    if (!x || !w || !scale || !shift || !y) return fail(CMK_EINVAL, "dwconv_bn_act: null pointer%s", "");
    if (N < 1 || H < 1 || W < 1 || C < 1) return fail(CMK_EINVAL, "dwconv_bn_act: empty shape%s (N, H, W, C must be >= 1)", "");
    if (const char* why = dw_view_error(x, x_cs, x_co, y, y_cs, y_co, C)) return fail(CMK_EINVAL, "dwconv_bn_act: %s (C = %ld)", why, (long)C);
    if (stride != 1 && stride != 2) return fail(CMK_EINVAL, "dwconv_bn_act: %sstride %ld must be 1 or 2", "", (long)stride);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)y) & 15)
        return fail(CMK_EINVAL, "dwconv_bn_act: pointers must be 16-byte aligned%s", "");
    if (in_max != in_max || out_min != out_min || out_max != out_max || out_min > out_max)
        return fail(CMK_EINVAL, "dwconv_bn_act: bad clamp bounds%s", "");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long)N * Ho * Wo * (C >> 2) > (1L << 31) - DW_MAX_GRID_STRIDE)
        return fail(CMK_EINVAL, "dwconv_bn_act: %s%ld output quads, the kernel indexes them in 32 bits with room for one grid stride", "", (long)N * Ho * Wo * (C >> 2));
    if (dw_overlap(x, x_co, y, y_co, C)) return fail(CMK_EINVAL, "dwconv_bn_act: input and output channel slices of one buffer overlap%s", "");
    const DwArgs a = {x, w, scale, shift, y, x_cs, x_co, y_cs, y_co, N, H, W, Ho, Wo, C >> 2, in_max, out_min, out_max, stream};
    // outputs per thread (T columns x R rows): the measured best tile while it still leaves >= 1024 workgroups (4 per CU), smaller on small maps
    if (stride == 1) {
        if (dw_blocks(a, 2, 4) >= 1024) launch_dw<1, 2, 4>(a);
        else if (dw_blocks(a, 4, 1) >= 1024) launch_dw<1, 4, 1>(a);
        else if (dw_blocks(a, 2, 1) >= 1024) launch_dw<1, 2, 1>(a);
        else launch_dw<1, 1, 1>(a);
    } else {
        if (dw_blocks(a, 2, 2) >= 1024) launch_dw<2, 2, 2>(a);
        else if (dw_blocks(a, 2, 1) >= 1024) launch_dw<2, 2, 1>(a);
        else launch_dw<2, 1, 1>(a);
    }
    return check_launch("dwconv3_bn_act");
}

extern "C" int cmk_dwconv3x3_nhwc(const float* x, int x_cs, int x_co, const float* w, float* y, int y_cs, int y_co, int N, int H, int W,
                                  int C, int stride, void* stream) {
    if (!x || !w || !y) return fail(CMK_EINVAL, "dwconv: null pointer%s", "");
    if (N < 1 || H < 1 || W < 1 || C < 1) return fail(CMK_EINVAL, "dwconv: empty shape%s (N, H, W, C must be >= 1)", "");
    if (const char* why = dw_view_error(x, x_cs, x_co, y, y_cs, y_co, C)) return fail(CMK_EINVAL, "dwconv: %s (C = %ld)", why, (long)C);
    if (stride != 1 && stride != 2) return fail(CMK_EINVAL, "dwconv: %sstride %ld must be 1 or 2", "", (long)stride);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) return fail(CMK_EINVAL, "dwconv: pointers must be 16-byte aligned%s", "");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long)N * Ho * Wo * (C >> 2) > (1L << 31) - DW_MAX_GRID_STRIDE)
        return fail(CMK_EINVAL, "dwconv: %s%ld output quads, the kernel indexes them in 32 bits with room for one grid stride", "", (long)N * Ho * Wo * (C >> 2));
    if (dw_overlap(x, x_co, y, y_co, C)) return fail(CMK_EINVAL, "dwconv: input and output channel slices of one buffer overlap%s", "");
    const DwArgs a = {x, w, nullptr, nullptr, y, x_cs, x_co, y_cs, y_co, N, H, W, Ho, Wo, C >> 2, INFINITY, -INFINITY, INFINITY, stream};
    if (stride == 1) launch_dw<1, 4, 1, true>(a);
    else launch_dw<2, 2, 1, true>(a);
    return check_launch("dwconv3");
}
