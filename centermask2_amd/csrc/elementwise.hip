// HBM-bound NHWC kernels of the backbone and the FPN: stem conv on the raw NCHW image, ceil-mode max pool,
// eSE (global average pool -> fc -> hsigmoid -> channel scale [+ identity]) and the FPN's 2x upsample + add.
// All of them move 16 bytes per lane (float4) with channels innermost, so a wave reads/writes whole 256 B-1 KiB runs.
#include "cmk_common.hpp"

namespace cmk {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Selects, not fmaxf / fminf (which return the other operand for a NaN): a NaN behaves as in torch.
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }   // max_pool2d: a NaN wins and stays
__device__ __forceinline__ float hsigmoid3(float v) {                                            // relu6(v) / 6 with v = fc + 3: a NaN stays
    v = v < 0.f ? 0.f : v;
    v = v > 6.f ? 6.f : v;
    return v / 6.0f;
}

// ---------------------------------------------------------------------------------------------------------------
// stem_1 (vovnet.py:409): conv3x3 s2 p1 on (N,3,H,W) NCHW -> (N,Ho,Wo,Cout) NHWC, y = relu(acc*scale + shift).
// 4 threads per output pixel, 16 output channels each (Cout = 64); 27 taps broadcast from LDS.
// ---------------------------------------------------------------------------------------------------------------
template <int NB>   // NB = Cout / 32
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       float* __restrict__ y, int N, int H, int W, int Ho, int Wo, long tiles) {
    // GEMM on the matrix pipe: M = output pixels (32 per wave tile), K = 27 taps padded to 28, N = Cout.
    // A[pixel][k] is gathered straight from the NCHW image (lane = pixel, lane>>5 = k parity), the 14 x NB weight
    // operands B[k][cout] stay in registers for the whole kernel, the accumulators come out with cout on the lane so
    // every store instruction writes two full 128-byte NHWC runs.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, hh = lane >> 5;
    constexpr int Cout = NB * 32;
    float b[14][NB], sc[NB], sh[NB];
    int dlt[14], khs[14], kws[14];
#pragma unroll
    for (int s = 0; s < 14; ++s) {
        const int k = 2 * s + hh;                 // tap index (kh*3+kw)*3+ci, 27 = padding
        const int ci = k % 3, t = k / 3, kw = t % 3, kh = t / 3;
        khs[s] = kh - 1; kws[s] = kw - 1;
        dlt[s] = (ci * H + kh - 1) * W + kw - 1;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b[s][nb] = k < 27 ? w[k * Cout + nb * 32 + li] : 0.f;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { sc[nb] = scale[nb * 32 + li]; sh[nb] = shift[nb * 32 + li]; }
    const long total = (long)N * Ho * Wo;
    const long hw = (long)Ho * Wo;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < tiles; tile += (long)gridDim.x * 4) {
        const long pix = tile * 32 + li;
        const bool pv = pix < total;
        const int n = (int)(pix / hw);
        const int rem = (int)(pix - (long)n * hw);
        const int oh = rem / Wo, ow = rem - oh * Wo;
        const int ih0 = oh * 2, iw0 = ow * 2;
        const float* xb = x + ((long)n * 3 * H + ih0) * W + iw0;
        float av[14];
#pragma unroll
        for (int s = 0; s < 14; ++s) {
            const int ih = ih0 + khs[s], iw = iw0 + kws[s];
            const bool ok = pv && (2 * s + hh < 27) && ih >= 0 && ih < H && iw >= 0 && iw < W;
            av[s] = ok ? xb[dlt[s]] : 0.f;
        }
        f32x16 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
#pragma unroll
        for (int s = 0; s < 14; ++s)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b[s][nb], acc[nb], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long op = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (op < total) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) y[op * Cout + nb * 32 + li] = fmaxf(acc[nb][r] * sc[nb] + sh[nb], 0.f);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, ceil_mode=True), no padding (vovnet.py:349-350).  One lane = one output pixel x 4 channels.
// ---------------------------------------------------------------------------------------------------------------
// A window that holds a NaN comes out NaN (F.max_pool2d), an all -inf window -inf.
// `gate` (optional, N*C, all >= 0): the eSE channel gate of the producer block applied after the max — max(x*g) == g*max(x)
// for g >= 0, so stage 2's eSE scale pass (whose output nobody else reads) folds into the pool.
__global__ __launch_bounds__(256) void maxpool3_kernel(const float* __restrict__ x, int x_cs, int x_co, float* __restrict__ y,
                                                      int y_cs, int y_co, int N, int H, int W, int Ho, int Wo, int C4,
                                                      const float* __restrict__ gate) {
    long total = (long)N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c4 = (int)(i % C4);
        long p = i / C4;
        int ow = (int)(p % Wo);
        int oh = (int)((p / Wo) % Ho);
        int n = (int)(p / ((long)Wo * Ho));
        f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                int ih = oh * 2 + kh, iw = ow * 2 + kw;
                if (ih < H && iw < W) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long)n * H + ih) * W + iw) * x_cs + x_co + c4 * 4);
                    m.x = nanmax(m.x, v.x); m.y = nanmax(m.y, v.y); m.z = nanmax(m.z, v.z); m.w = nanmax(m.w, v.w);
                }
            }
        if (gate) {
            f32x4 g = *reinterpret_cast<const f32x4*>(gate + ((long)n * C4 + c4) * 4);
            m.x *= g.x; m.y *= g.y; m.z *= g.z; m.w *= g.w;
        }
        *reinterpret_cast<f32x4*>(y + p * y_cs + y_co + c4 * 4) = m;
    }
}

// MaxPool2d(kernel 1, stride 2) = every second pixel (d2's LastLevelMaxPool, the top block of build_vovnet_fpn_backbone vovnet.py:504-524)
__global__ __launch_bounds__(256) void subsample2_kernel(const float* __restrict__ x, int x_cs, int x_co, float* __restrict__ y, int y_cs, int y_co,
                                                        int N, int H, int W, int Ho, int Wo, int C4) {
    long total = (long)N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c4 = (int)(i % C4);
        long p = i / C4;
        int ow = (int)(p % Wo);
        int oh = (int)((p / Wo) % Ho);
        int n = (int)(p / ((long)Wo * Ho));
        *reinterpret_cast<f32x4*>(y + p * y_cs + y_co + c4 * 4) =
            *reinterpret_cast<const f32x4*>(x + (((long)n * H + 2 * oh) * W + 2 * ow) * x_cs + x_co + c4 * 4);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// eSE (vovnet.py:247-260).  Stage 1: per (image, pixel chunk) channel sums (deterministic: fixed order, no atomics).
// Stage 2: mean -> fc (C x C mat-vec, one wave per output, wave64 shuffle reduction) -> relu6(v+3)/6.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ese_partial_kernel(const float* __restrict__ x, int x_cs, int x_co, float* __restrict__ ws,
                                                         int HW, int C, int chunks) {
    extern __shared__ float red[];  // [ppl][C]
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int G = C >> 2;
    const int ppl = G >= 256 ? 1 : 256 / G;  // pixel lanes that share a channel group
    const int per = cdiv(HW, chunks);
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    const float* xn = x + (long)n * HW * x_cs + x_co;
    for (int gi = threadIdx.x; gi < G * ppl; gi += 256) {
        int g = gi % G, pl = gi / G;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int p = p0 + pl; p < p1; p += ppl) {
            f32x4 v = *reinterpret_cast<const f32x4*>(xn + (long)p * x_cs + g * 4);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<f32x4*>(red + pl * C + g * 4) = s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int pl = 0; pl < ppl; ++pl) s += red[pl * C + c];
        ws[((long)n * chunks + chunk) * C + c] = s;
    }
}

__global__ __launch_bounds__(256) void ese_fc_kernel(const float* __restrict__ ws, const float* __restrict__ fc_w,
                                                    const float* __restrict__ fc_b, float* __restrict__ gate, int HW, int C,
                                                    int chunks) {
    // 16 outputs per workgroup.  Stage 1 reduces the per-chunk partial sums to the channel means: the chunk range is split over
    // `parts` thread groups (16 B per thread per chunk, independent loads), folded through LDS.  Stage 2: one wave per output.
    // (float64 from the partial sums on, as in ese_fc_pooled_kernel)
    extern __shared__ double smd[];  // [parts][C] partials, then mean in row 0
    const int n = blockIdx.y;
    const int G = C >> 2;
    const int parts = G >= 256 ? 1 : 256 / G;
    const float* wsn = ws + (long)n * chunks * C;
    for (int gi = threadIdx.x; gi < G * parts; gi += 256) {
        const int g = gi % G, part = gi / G;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 8
        for (int k = part; k < chunks; k += parts) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(wsn + (long)k * C + g * 4);
            s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        }
        double* o = smd + part * C + g * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int part = 0; part < parts; ++part) s += smd[part * C + c];
        smd[c] = s / (double)HW;   // row 0 is only read by its own thread above
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = blockIdx.x * 16 + wave; o < min(C, (int)(blockIdx.x + 1) * 16); o += 4) {
        const float* wr = fc_w + (long)o * C;
        double s = 0.0;
        for (int c = lane * 4; c < C; c += 256) {
            f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c);
            s += (double)wv.x * smd[c] + (double)wv.y * smd[c + 1] + (double)wv.z * smd[c + 2] + (double)wv.w * smd[c + 3];
        }
        s = wave_sum(s);
        if (lane == 0) {
            float v = (float)(s + (double)fc_b[o] + 3.0);
            gate[(long)n * C + o] = hsigmoid3(v);      // a NaN mean gives a NaN gate: the image comes out NaN, as in torch
        }
    }
}

// The gate from the per-block sums the aggregation conv left behind (cmk_conv_desc.pool_ws): record 2g = rows of block g in the image of
// its first pixel, 2g+1 = rows of block g in the next image.  Stage 1 (channel means) differs from ese_fc_kernel, stage 2 is the same.
__global__ __launch_bounds__(256) void ese_fc_pooled_kernel(const float* __restrict__ rec, int rows, const float* __restrict__ fc_w,
                                                           const float* __restrict__ fc_b, float* __restrict__ gate, int HW, int C) {
    // The records are fp32 sums of at most `rows` values each; everything downstream of them — the sum over the records, the mean and
    // the C x C fully-connected layer — is accumulated in float64 in a fixed order (a few thousand adds per image: free), so the gate
    // carries the rounding of the records and of one final conversion only (the detection order of near-tied scores
    // depends on summation-order noise upstream; this removes this kernel's share of it).
    extern __shared__ double smd[];  // [parts][C] partials, then the mean in row 0
    const int n = blockIdx.y;
    const int G = C >> 2;
    const int parts = G >= 256 ? 1 : 256 / G;
    const long p0 = (long)n * HW;
    const long g0 = p0 / rows, g1 = (p0 + HW - 1) / rows;
    const long first = (g0 * rows == p0) ? 2 * g0 : 2 * g0 + 1;          // the record of block g0 that holds this image's rows
    for (int gi = threadIdx.x; gi < G * parts; gi += 256) {
        const int g = gi % G, part = gi / G;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (part == 0) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(rec + first * C + g * 4);
            s0 = v.x; s1 = v.y; s2 = v.z; s3 = v.w;
        }
#pragma unroll 8
        for (long k = g0 + 1 + part; k <= g1; k += parts) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(rec + 2 * k * C + g * 4);
            s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        }
        double* o = smd + part * C + g * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int part = 0; part < parts; ++part) s += smd[part * C + c];
        smd[c] = s / (double)HW;   // row 0 is only read by its own thread above
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = blockIdx.x * 16 + wave; o < min(C, (int)(blockIdx.x + 1) * 16); o += 4) {
        const float* wr = fc_w + (long)o * C;
        double s = 0.0;
        for (int c = lane * 4; c < C; c += 256) {
            f32x4 wv = *reinterpret_cast<const f32x4*>(wr + c);
            s += (double)wv.x * smd[c] + (double)wv.y * smd[c + 1] + (double)wv.z * smd[c + 2] + (double)wv.w * smd[c + 3];
        }
        s = wave_sum(s);
        if (lane == 0) {
            float v = (float)(s + (double)fc_b[o] + 3.0);
            gate[(long)n * C + o] = hsigmoid3(v);      // a NaN mean gives a NaN gate: the image comes out NaN, as in torch
        }
    }
}

__global__ __launch_bounds__(256) void ese_scale_kernel(const float* __restrict__ x, int x_cs, int x_co, const float* __restrict__ gate,
                                                       const float* __restrict__ idn, int id_cs, int id_co, float* __restrict__ y,
                                                       int y_cs, int y_co, int N, int HW, int C4) {
    long total = (long)N * HW * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c4 = (int)(i % C4);
        long p = i / C4;
        int n = (int)(p / HW);
        f32x4 v = *reinterpret_cast<const f32x4*>(x + p * x_cs + x_co + c4 * 4);
        f32x4 g = *reinterpret_cast<const f32x4*>(gate + (long)n * C4 * 4 + c4 * 4);
        f32x4 o = {v.x * g.x, v.y * g.y, v.z * g.z, v.w * g.w};
        if (idn) {
            f32x4 d = *reinterpret_cast<const f32x4*>(idn + p * id_cs + id_co + c4 * 4);
            o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w;
        }
        *reinterpret_cast<f32x4*>(y + p * y_cs + y_co + c4 * 4) = o;
    }
}

// nearest-neighbour 2x upsampling of `coarse` added to `y` in place (d2 FPN's top-down path, ctor at vovnet.py:547-554, when a norm sits between the
// lateral conv and the sum, so that the sum cannot ride in the conv's epilogue)
__global__ __launch_bounds__(256) void upsample2x_add_kernel(float* __restrict__ y, const float* __restrict__ c, int N, int H, int W, int Hc, int Wc, int C4) {
    long total = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int c4 = (int)(i % C4);
        long p = i / C4;
        int w = (int)(p % W);
        int h = (int)((p / W) % H);
        int n = (int)(p / ((long)W * H));
        const f32x4 a = *reinterpret_cast<const f32x4*>(y + i * 4);
        const f32x4 b = *reinterpret_cast<const f32x4*>(c + ((((long)n * Hc + (h >> 1)) * Wc + (w >> 1)) * C4 + c4) * 4);
        *reinterpret_cast<f32x4*>(y + i * 4) = f32x4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
    }
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_stem_conv_nchw3(const float* x, const float* w, const float* scale, const float* shift, float* y, int N, int H,
                                   int W, int Cout, void* stream) {
    if (!x || !w || !scale || !shift || !y) return fail(CMK_EINVAL, "stem: null pointer%s", "");
    if (Cout != 32 && Cout != 64 && Cout != 128) return fail(CMK_EINVAL, "stem: Cout (%s%ld) must be 32, 64 or 128", "", (long)Cout);
    int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    long total = (long)N * Ho * Wo;
    if ((long)3 * H * W >= (1L << 31)) return fail(CMK_EINVAL, "stem: image too large%s", "");
    long tiles = (total + 31) / 32;
    unsigned grid = (unsigned)std::min<long>((tiles + 3) / 4, 256 * 16);
    if (Cout == 32)
        hipLaunchKernelGGL(stem_conv_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift, y, N, H, W, Ho, Wo, tiles);
    else if (Cout == 64)
        hipLaunchKernelGGL(stem_conv_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift, y, N, H, W, Ho, Wo, tiles);
    else
        hipLaunchKernelGGL(stem_conv_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift, y, N, H, W, Ho, Wo, tiles);
    return check_launch("stem_conv");
}

extern "C" int cmk_maxpool3x3s2_ceil_nhwc(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co, int N, int H, int W, int C,
                                          const float* gate, void* stream) {
    if (!x || !y) return fail(CMK_EINVAL, "maxpool: null pointer%s", "");
    if ((C & 3) || (x_cs & 3) || (x_co & 3) || (y_cs & 3) || (y_co & 3)) return fail(CMK_EINVAL, "maxpool: channels must be multiples of 4%s", "");
    if (H < 3 || W < 3) return fail(CMK_EINVAL, "maxpool: input smaller than the window%s", "");
    int Ho = (H - 3 + 1) / 2 + 1, Wo = (W - 3 + 1) / 2 + 1;  // ceil((H-3)/2)+1
    if ((Ho - 1) * 2 >= H) --Ho;
    if ((Wo - 1) * 2 >= W) --Wo;
    long total = (long)N * Ho * Wo * (C >> 2);
    hipLaunchKernelGGL(maxpool3_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, x_cs, x_co, y, y_cs, y_co, N, H, W,
                       Ho, Wo, C >> 2, gate);
    return check_launch("maxpool3");
}

extern "C" int cmk_maxpool1x1s2_nhwc(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co, int N, int H, int W, int C, void* stream) {
    if (!x || !y) return fail(CMK_EINVAL, "maxpool1x1s2: null pointer%s", "");
    if ((C & 3) || (x_cs & 3) || (x_co & 3) || (y_cs & 3) || (y_co & 3) || N < 1 || H < 1 || W < 1)
        return fail(CMK_EINVAL, "maxpool1x1s2: channels must be multiples of 4, N, H, W >= 1%s", "");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    long total = (long)N * Ho * Wo * (C >> 2);
    hipLaunchKernelGGL(subsample2_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, x_cs, x_co, y, y_cs, y_co, N, H, W, Ho, Wo,
                       C >> 2);
    return check_launch("maxpool1x1s2");
}

extern "C" int cmk_ese_gate(const float* x, int x_cs, int x_co, const float* fc_w, const float* fc_b, float* gate, float* ws,
                            int ws_chunks, int N, int HW, int C, void* stream) {
    if (!x || !fc_w || !fc_b || !gate || !ws) return fail(CMK_EINVAL, "ese_gate: null pointer%s", "");
    if ((C & 3) || (x_cs & 3) || (x_co & 3) || ws_chunks < 1) return fail(CMK_EINVAL, "ese_gate: bad shape%s", "");
    if (N < 1 || HW < 1 || C < 4) return fail(CMK_EINVAL, "ese_gate: N, H*W >= 1 and C >= 4%s", "");
    int G = C >> 2;
    int ppl = G >= 256 ? 1 : 256 / G;
    size_t lds1 = (size_t)ppl * C * sizeof(float);
    hipLaunchKernelGGL(ese_partial_kernel, dim3(ws_chunks, N), dim3(256), lds1, (hipStream_t)stream, x, x_cs, x_co, ws, HW, C, ws_chunks);
    int rc = check_launch("ese_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(ese_fc_kernel, dim3(cdiv(C, 16), N), dim3(256), 2 * lds1 /* doubles */, (hipStream_t)stream, ws, fc_w, fc_b,
                       gate, HW, C, ws_chunks);
    return check_launch("ese_fc");
}

extern "C" int cmk_ese_gate_pooled(const float* pool_ws, int rows, const float* fc_w, const float* fc_b, float* gate, int N, int HW, int C, void* stream) {
    if (!pool_ws || !fc_w || !fc_b || !gate) return fail(CMK_EINVAL, "ese_gate_pooled: null pointer%s", "");
    if ((C & 3) || C < 4 || rows < 1 || HW < rows || N < 1) return fail(CMK_EINVAL, "ese_gate_pooled: bad shape (C %% 4, H*W >= rows)%s", "");
    const int G = C >> 2;
    const int parts = G >= 256 ? 1 : 256 / G;
    hipLaunchKernelGGL(ese_fc_pooled_kernel, dim3(cdiv(C, 16), N), dim3(256), (size_t)parts * C * sizeof(double), (hipStream_t)stream, pool_ws, rows,
                       fc_w, fc_b, gate, HW, C);
    return check_launch("ese_fc_pooled");
}

extern "C" int cmk_ese_scale(const float* x, int x_cs, int x_co, const float* gate, const float* identity, int id_cs, int id_co, float* y,
                             int y_cs, int y_co, int N, int HW, int C, void* stream) {
    if (!x || !gate || !y) return fail(CMK_EINVAL, "ese_scale: null pointer%s", "");
    if ((C & 3) || (x_cs & 3) || (x_co & 3) || (y_cs & 3) || (y_co & 3) || (id_cs & 3) || (id_co & 3))
        return fail(CMK_EINVAL, "ese_scale: channels must be multiples of 4%s", "");
    if (N < 1 || HW < 1) return fail(CMK_EINVAL, "ese_scale: N, H*W >= 1%s", "");
    long total = (long)N * HW * (C >> 2);
    hipLaunchKernelGGL(ese_scale_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, x_cs, x_co, gate, identity, id_cs,
                       id_co, y, y_cs, y_co, N, HW, C >> 2);
    return check_launch("ese_scale");
}

extern "C" int cmk_upsample2x_add_nhwc(float* y, const float* coarse, int N, int H, int W, int Hc, int Wc, int C, void* stream) {
    if (!y || !coarse) return fail(CMK_EINVAL, "upsample2x_add: null pointer%s", "");
    if ((C & 3) || N < 1 || H < 1 || W < 1 || Hc * 2 < H || Wc * 2 < W) return fail(CMK_EINVAL, "upsample2x_add: C %% 4 == 0 and a coarse map of at least half the size%s", "");
    long total = (long)N * H * W * (C >> 2);
    hipLaunchKernelGGL(upsample2x_add_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, y, coarse, N, H, W, Hc, Wc, C >> 2);
    return check_launch("upsample2x_add");
}
