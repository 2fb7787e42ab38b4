// Grouped 3x3 conv of a ResNeXt bottleneck (detectron2 BottleneckBlock.conv2 with MODEL.RESNETS.NUM_GROUPS > 1) with its FrozenBN folded:
//   y = [relu](gconv3x3(x) * scale[c] + shift[c])        pad 1, stride 1 | 2, no bias, Cin = Cout = C, `groups` groups of Cg = C / groups,
// NHWC channel-slice views.  Exact fp32: fp32 products, fp32 accumulation (an fmaf chain per output, on the VALU or inside the f32 MFMA).
// A group reads only its own Cg input channels, so a NaN or Inf in one group never reaches another group's outputs; the zero padding is
// zeros of the input.  The ReLU is a select: a NaN passes through as in torch.
//
// Two kernels, chosen by Cg:
//   Cg in {16, 32, 64}: group3_mfma_kernel, v_mfma_f32_16x16x4_f32 with the WEIGHTS as the A operand (16 couts of one group per N-tile of
//     the group, Cg/16 tiles) and 16 adjacent output pixels of one row as the B operand, so a lane ends with 4 consecutive couts of one pixel
//     and stores 16 bytes.  A workgroup (4 waves) is one group x one output tile of TH x 16 pixels (TH = 8 at stride 1, 4 at stride 2; a wave
//     owns TH/4 rows and every cout tile).  K runs over 16-channel chunks of the group: per chunk the input halo tile ((TH-1)S+3 rows x
//     15S+3 columns x 16 channels) and the chunk's 9 x 16 x Cg weights are staged in LDS once, then every tap is Cg/16 + TH/4 ds_read_b128
//     and 4 * Cg/16 * TH/4 MFMAs per wave.  The halo tile is stored as four planes, one per 4-channel quarter (plane size a multiple of
//     256 bytes), and at stride 2 with its even columns before its odd ones, so the 16 pixels of a tap are contiguous in every plane and
//     the 128-bit reads are conflict-free.  The k order inside a chunk is free: MFMA j of a chunk takes channel 4q + j from lane quarter q,
//     which is what one 16-byte read per lane delivers.
//   Cg in {4, 8}: group3_valu_kernel, register-tiled like dwconv_bn_act.hip: one thread = 4 couts x T columns x R rows, lanes along the
//     channel quads so input and weight reads are contiguous, T x R = 2 x 2 at stride 1 and 4 x 2 at stride 2; the Cg/4 input quads of
//     the thread's group are read per tap row, the weights (12 quads per tap row and input quad) come through the L1: a workgroup is 16
//     channel quads x 16 adjacent pixel tiles, so the weights it touches (9 * Cg * 64 floats, 18 KiB at Cg = 8) fit the L1.
// No workspace, no memset, one launch.
//
// Weight packing (ops.pack_group_weight, weight (C, Cg, 3, 3), tap = kh*3 + kw, ci the input channel inside the group):
//   Cg in {4, 8}:        [tap][ci][C]                                  packed[(tap*Cg + ci)*C + cout] = weight[cout][ci][kh][kw]
//   Cg in {16, 32, 64}:  [group][chunk][tap][tile][q][n][j], 4-float j innermost: the element is
//                        weight[group*Cg + tile*16 + n][chunk*16 + 4*q + j][kh][kw],   chunk < Cg/16, tile < Cg/16, q < 4, n < 16, j < 4,
//                        i.e. per (group, chunk, tap, tile) the 64 A-operand quads in lane order (lane = q*16 + n).
#include "cmk_common.hpp"

namespace cmk {
namespace {

typedef float gq __attribute__((ext_vector_type(4)));

__device__ inline float relu_sel(float v, int relu) { return (relu && v < 0.f) ? 0.f : v; }      // NaN stays NaN

template <int S>
struct MfmaTile {
    static constexpr int TW = 16, TH = S == 1 ? 8 : 4, PT = TH / 4;
    static constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;       // 10 x 18 | 9 x 33
    static constexpr int EVEN = (IW + 1) / 2;                                // stride 2: the even columns come first
    static constexpr int PLANE = (IH * IW + 15) / 16 * 16;                   // quads; a multiple of 256 bytes
};

template <int CG, int S>
__global__ __launch_bounds__(256) void group3_mfma_kernel(const float* __restrict__ x, int x_cs, int x_co, const float* __restrict__ w,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         float* __restrict__ y, int y_cs, int y_co, int H, int W, int Ho, int Wo, int groups,
                                                         int HT, int WT, int relu) {
    using TL = MfmaTile<S>;
    constexpr int TW = TL::TW, TH = TL::TH, PT = TL::PT, IH = TL::IH, IW = TL::IW, EVEN = TL::EVEN, PLANE = TL::PLANE;
    constexpr int NT = CG / 16, NCH = CG / 16, WQ = 9 * NT * 64;             // weight quads per chunk
    __shared__ gq sx[4 * PLANE];
    __shared__ gq sw[WQ];
    int bid = blockIdx.x;                                                   // < 2^31, checked on the host
    const int g = bid % groups;
    bid /= groups;
    const int wt = bid % WT;
    bid /= WT;
    const int ht = bid % HT, n = bid / HT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, q = lane >> 4;
    const int oh0 = ht * TH, ow0 = wt * TW, ih0 = oh0 * S - 1, iw0 = ow0 * S - 1;
    gq acc[NT][PT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < PT; ++r) acc[t][r] = gq{0.f, 0.f, 0.f, 0.f};
    const float* xg = x + x_co + g * CG;
    const gq* wg = reinterpret_cast<const gq*>(w) + (long)g * NCH * WQ;
    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        for (int i = tid; i < IH * IW * 4; i += 256) {
            const int qq = i & 3, pix = i >> 2, r = pix / IW, c = pix % IW;
            const int ih = ih0 + r, iw = iw0 + c;
            gq v = {0.f, 0.f, 0.f, 0.f};
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = *reinterpret_cast<const gq*>(xg + (((long)n * H + ih) * W + iw) * x_cs + ch * 16 + qq * 4);
            const int slot = S == 1 ? c : (c & 1) * EVEN + (c >> 1);
            sx[qq * PLANE + r * IW + slot] = v;
        }
        for (int i = tid; i < WQ; i += 256) sw[i] = wg[(long)ch * WQ + i];
        __syncthreads();
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                gq b[PT];
#pragma unroll
                for (int r = 0; r < PT; ++r) {
                    const int row = (wave * PT + r) * S + kh;
                    const int slot = S == 1 ? p + kw : (kw & 1) * EVEN + p + (kw >> 1);
                    b[r] = sx[q * PLANE + row * IW + slot];
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const gq a = sw[((kh * 3 + kw) * NT + t) * 64 + lane];
#pragma unroll
                    for (int r = 0; r < PT; ++r) {
                        acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[r].x, acc[t][r], 0, 0, 0);
                        acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[r].y, acc[t][r], 0, 0, 0);
                        acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[r].z, acc[t][r], 0, 0, 0);
                        acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[r].w, acc[t][r], 0, 0, 0);
                    }
                }
            }
    }
    // D: column (lane & 15) is the pixel, row 4q + reg the cout inside the tile -> one 16-byte store per lane and tile
    const int ow = ow0 + p;
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int oh = oh0 + wave * PT + r;
        if (oh >= Ho || ow >= Wo) continue;
        float* yp = y + (((long)n * Ho + oh) * Wo + ow) * y_cs + y_co;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = g * CG + t * 16 + q * 4;
            const gq sc = *reinterpret_cast<const gq*>(scale + c), sh = *reinterpret_cast<const gq*>(shift + c);
            gq o = acc[t][r];
            o.x = relu_sel(fmaf(o.x, sc.x, sh.x), relu);
            o.y = relu_sel(fmaf(o.y, sc.y, sh.y), relu);
            o.z = relu_sel(fmaf(o.z, sc.z, sh.z), relu);
            o.w = relu_sel(fmaf(o.w, sc.w, sh.w), relu);
            *reinterpret_cast<gq*>(yp + c) = o;
        }
    }
}

template <int CG, int S, int T, int R>
__global__ __launch_bounds__(256) void group3_valu_kernel(const float* __restrict__ x, int x_cs, int x_co, const float* __restrict__ w,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         float* __restrict__ y, int y_cs, int y_co, int N, int H, int W, int Ho, int Wo, int C4,
                                                         int relu) {
    constexpr int COLS = (T - 1) * S + 3, Q = CG / 4;
    const int WT = (Wo + T - 1) / T, HT = (Ho + R - 1) / R;
    const int tiles = N * HT * WT, chunks = (C4 + 15) >> 4;      // tiles * C4 < 2^31, checked on the host
    const long total = (long)((tiles + 15) >> 4) * chunks * 256;
    const gq* wq4 = reinterpret_cast<const gq*>(w);
    // a workgroup is 16 channel quads x 16 adjacent pixel tiles (quad fastest, 4 tiles per wave): its weights, 9 * Cg * 64 floats, stay in the L1
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long wg = i >> 8;
        const int c4 = (int)(wg % chunks) * 16 + (threadIdx.x & 15);
        int rem = (int)(wg / chunks) * 16 + (threadIdx.x >> 4);
        if (c4 >= C4 || rem >= tiles) continue;
        const int wt = rem % WT;
        rem /= WT;
        const int ht = rem % HT, n = rem / HT;
        const int gin = c4 / Q * CG;                  // first input channel of this thread's group
        const int oh0 = ht * R, iw0 = wt * T * S - 1;
        gq acc[R][T];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < T; ++j) acc[r][j] = gq{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cq = 0; cq < Q; ++cq) {
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                gq wv[3][4];                          // [kw][ci inside the quad]: the thread's 4 couts
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int e = 0; e < 4; ++e) wv[kw][e] = wq4[((long)(kh * 3 + kw) * CG + cq * 4 + e) * C4 + c4];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int ih = (oh0 + r) * S - 1 + kh;
                    if (ih < 0 || ih >= H) continue;
                    const float* row = x + ((long)n * H + ih) * W * x_cs + x_co + gin + cq * 4;
#pragma unroll
                    for (int cc = 0; cc < COLS; ++cc) {
                        const int iw = iw0 + cc;
                        gq v = {0.f, 0.f, 0.f, 0.f};
                        if (iw >= 0 && iw < W) v = *reinterpret_cast<const gq*>(row + (long)iw * x_cs);
#pragma unroll
                        for (int j = 0; j < T; ++j) {
                            const int kw = cc - j * S;       // compile-time after unrolling
                            if (kw < 0 || kw >= 3) continue;
                            gq a = acc[r][j];
                            const gq w0 = wv[kw][0], w1 = wv[kw][1], w2 = wv[kw][2], w3 = wv[kw][3];
                            a.x = fmaf(v.x, w0.x, a.x); a.y = fmaf(v.x, w0.y, a.y); a.z = fmaf(v.x, w0.z, a.z); a.w = fmaf(v.x, w0.w, a.w);
                            a.x = fmaf(v.y, w1.x, a.x); a.y = fmaf(v.y, w1.y, a.y); a.z = fmaf(v.y, w1.z, a.z); a.w = fmaf(v.y, w1.w, a.w);
                            a.x = fmaf(v.z, w2.x, a.x); a.y = fmaf(v.z, w2.y, a.y); a.z = fmaf(v.z, w2.z, a.z); a.w = fmaf(v.z, w2.w, a.w);
                            a.x = fmaf(v.w, w3.x, a.x); a.y = fmaf(v.w, w3.y, a.y); a.z = fmaf(v.w, w3.z, a.z); a.w = fmaf(v.w, w3.w, a.w);
                            acc[r][j] = a;
                        }
                    }
                }
            }
        }
        const gq sc = *reinterpret_cast<const gq*>(scale + c4 * 4), sh = *reinterpret_cast<const gq*>(shift + c4 * 4);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int oh = oh0 + r;
            if (oh >= Ho) continue;
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const int ow = wt * T + j;
                if (ow >= Wo) continue;
                gq o = acc[r][j];
                o.x = relu_sel(fmaf(o.x, sc.x, sh.x), relu);
                o.y = relu_sel(fmaf(o.y, sc.y, sh.y), relu);
                o.z = relu_sel(fmaf(o.z, sc.z, sh.z), relu);
                o.w = relu_sel(fmaf(o.w, sc.w, sh.w), relu);
                *reinterpret_cast<gq*>(y + (((long)n * Ho + oh) * Wo + ow) * y_cs + y_co + c4 * 4) = o;
            }
        }
    }
}

struct GroupArgs {
    const float *x, *w, *scale, *shift;
    float* y;
    int x_cs, x_co, y_cs, y_co, N, H, W, Ho, Wo, C, groups, relu;
    void* stream;
};

template <int CG, int S>
void launch_mfma(const GroupArgs& a) {
    using TL = MfmaTile<S>;
    const int HT = cdiv(a.Ho, TL::TH), WT = cdiv(a.Wo, TL::TW);
    const unsigned grid = (unsigned)((long)a.N * HT * WT * a.groups);
    hipLaunchKernelGGL((group3_mfma_kernel<CG, S>), dim3(grid), dim3(256), 0, (hipStream_t)a.stream, a.x, a.x_cs, a.x_co, a.w, a.scale, a.shift, a.y,
                       a.y_cs, a.y_co, a.H, a.W, a.Ho, a.Wo, a.groups, HT, WT, a.relu);
}

template <int CG, int S, int T, int R>
void launch_valu_tile(const GroupArgs& a) {
    const long blocks = (((long)a.N * cdiv(a.Ho, R) * cdiv(a.Wo, T) + 15) >> 4) * (((a.C >> 2) + 15) >> 4);
    const unsigned grid = (unsigned)(blocks > 16384 ? 16384 : blocks);
    hipLaunchKernelGGL((group3_valu_kernel<CG, S, T, R>), dim3(grid), dim3(256), 0, (hipStream_t)a.stream, a.x, a.x_cs, a.x_co, a.w, a.scale, a.shift,
                       a.y, a.y_cs, a.y_co, a.N, a.H, a.W, a.Ho, a.Wo, a.C >> 2, a.relu);
}

// one thread tile per stride, 2 rows x 2 columns at stride 1 (the best of six tiles measured at the 8 x 200 x 320 x 256 layer) and 2 x 4 at stride 2
template <int CG>
void launch_valu(const GroupArgs& a, int stride) {
    if (stride == 1) launch_valu_tile<CG, 1, 2, 2>(a);
    else launch_valu_tile<CG, 2, 4, 2>(a);
}

template <int CG>
void launch_mfma_stride(const GroupArgs& a, int stride) {
    if (stride == 1) launch_mfma<CG, 1>(a);
    else launch_mfma<CG, 2>(a);
}

}  // namespace
}  // namespace cmk

using namespace cmk;

extern "C" int cmk_group_conv3x3_nhwc(const float* x, int x_cs, int x_co, const float* w, const float* scale, const float* shift, float* y,
                                      int y_cs, int y_co, int N, int H, int W, int C, int groups, int stride, int relu, void* stream) {
    if (!x || !w || !scale || !shift || !y) return fail(CMK_EINVAL, "group_conv3x3: null pointer%s", "");
    if (N < 1 || H < 1 || W < 1 || C < 1) return fail(CMK_EINVAL, "group_conv3x3: empty shape%s (N, H, W, C must be >= 1)", "");
    if (groups < 2 || C % groups) return fail(CMK_EINVAL, "group_conv3x3: %sC = %ld must be divisible by groups = %ld >= 2", "", (long)C, (long)groups);
    const int cg = C / groups;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64)
        return fail(CMK_EINVAL, "group_conv3x3: %sCg = %ld channels per group is not built (4, 8, 16, 32 and 64 are)", "", (long)cg);
    if (stride != 1 && stride != 2) return fail(CMK_EINVAL, "group_conv3x3: %sstride %ld must be 1 or 2", "", (long)stride);
    if ((x_cs & 3) || (x_co & 3) || (y_cs & 3) || (y_co & 3) || x_co < 0 || y_co < 0)
        return fail(CMK_EINVAL, "group_conv3x3: misaligned channel offset or pixel stride%s (x %ld, y %ld: multiples of 4 floats)", "", (long)x_co, (long)y_co);
    if ((long)x_co + C > x_cs || (long)y_co + C > y_cs) return fail(CMK_EINVAL, "group_conv3x3: channel slice%s [co, co + %ld) leaves the pixel", "", (long)C);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)y) & 15)
        return fail(CMK_EINVAL, "group_conv3x3: pointers must be 16-byte aligned%s", "");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long)N * Ho * Wo * (C >> 2) >= (1L << 31))
        return fail(CMK_EINVAL, "group_conv3x3: %s%ld output quads, the kernel indexes them in 32 bits", "", (long)N * Ho * Wo * (C >> 2));
    if (x == y && x_co < y_co + C && y_co < x_co + C)
        return fail(CMK_EINVAL, "group_conv3x3: input and output channel slices of one buffer overlap%s", "");
    const GroupArgs a = {x, w, scale, shift, y, x_cs, x_co, y_cs, y_co, N, H, W, Ho, Wo, C, groups, relu ? 1 : 0, stream};
    switch (cg) {
        case 4: launch_valu<4>(a, stride); break;
        case 8: launch_valu<8>(a, stride); break;
        case 16: launch_mfma_stride<16>(a, stride); break;
        case 32: launch_mfma_stride<32>(a, stride); break;
        default: launch_mfma_stride<64>(a, stride); break;
    }
    return check_launch("group_conv3x3");
}
