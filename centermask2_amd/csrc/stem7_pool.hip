// d2 BasicStem of a ResNet in ONE launch: conv 7x7 stride 2 pad 3 on the NCHW 3-channel image, FrozenBN (folded), ReLU and
// max_pool2d(kernel 3, stride 2, padding 1), NHWC out.  The (N, H/2, W/2, 64) conv map never goes to HBM.
//
// Form: a conv tile with a one-pixel halo in LDS.  A workgroup (4 waves) owns S7_PH x S7_PW = 4 x 6 pooled pixels of one image.  It
//   1. stages the 23 x 31 x 3 input patch those need into LDS (zeros outside the image, columns split into an even and an odd half so
//      that the stride-2 walk of the conv reads consecutive words),
//   2. computes the 9 x 13 = 117 conv pixels under the 24 pooling windows as a GEMM on the matrix pipe, M = 4 x 32 conv pixels (one
//      32-row tile per wave, 11 rows idle), K = 147 taps padded to 148 (ordered by s7_step), N = 64 couts, v_mfma_f32_32x32x2_f32
//      with the 74 x 2 weight operands in registers for the whole (persistent) kernel, and writes relu(acc * scale + shift) to LDS,
//      -inf for the conv pixels that lie outside the conv map (pool padding never wins),
//   3. takes the 3 x 3 max per pooled pixel from LDS and stores float4s of the NHWC output view.
// Recompute: 117 conv pixels are computed for the 96 (= 8 x 12) a tile owns, 1.22x; the matrix pipe runs 128 rows for them, 1.33x.
// A NaN behaves as in torch: relu keeps it, the max returns it for every window that holds it.
#include "cmk_common.hpp"

namespace cmk {

typedef float s7_f32x4 __attribute__((ext_vector_type(4)));
typedef float s7_f32x16 __attribute__((ext_vector_type(16)));

constexpr int S7_PH = 4, S7_PW = 6;                        // pooled pixels per workgroup
constexpr int S7_CR = 2 * S7_PH + 1, S7_CC = 2 * S7_PW + 1; // conv pixels under them: 9 x 13
constexpr int S7_CPIX = S7_CR * S7_CC;                     // 117 <= 128 = 4 waves x 32 GEMM rows
constexpr int S7_IR = 2 * S7_CR + 5, S7_IC = 2 * S7_CC + 5; // input patch: 23 x 31
constexpr int S7_HALF = (S7_IC + 1) / 2;                   // 16 even columns, then 15 odd ones
constexpr int S7_IP = 39;                                  // input row pitch (>= 2 * S7_HALF; 2 * 39 % 32 = 14 spreads the rows of a wave over the banks)
constexpr int S7_PLANE = S7_IR * S7_IP;
constexpr int S7_OP = 68;                                  // floats per conv pixel in LDS (64 couts + 4: the two half-waves write rows 4 apart)
constexpr int S7_KS = 74;                                  // K steps of 2
static_assert(S7_CPIX <= 128 && S7_IP >= 2 * S7_HALF, "stem7 tile");

// K order of the GEMM.  A step feeds two taps to the matrix pipe, the first from lanes 0-31 and the second from lanes 32-63.  The taps are
// paired so that the second sits a fixed distance from the first in the LDS patch and every read is `lane base + immediate`:
//   steps 0-62: (ci, kh, kw = 0|2|4) and its right neighbour kw + 1 (S7_HALF further: the odd columns);
//   steps 63-71: (ci, kh = 0|2|4, kw = 6) and the tap one row down (S7_IP further);
//   step 72: (ci = 0, kh = 6, kw = 6) and the same tap of ci = 1 (S7_PLANE further);  step 73: (ci = 2, 6, 6) alone.
struct S7Step { int k0, k1, off, kind; };    // weight rows k = (kh*7 + kw)*3 + ci of the two taps (-1: none), patch offset of the first, distance kind
__host__ __device__ constexpr S7Step s7_step(int s) {
    if (s < 63) {
        const int ci = s / 21, kh = (s % 21) / 3, j = s % 3;
        return {(kh * 7 + 2 * j) * 3 + ci, (kh * 7 + 2 * j + 1) * 3 + ci, ci * S7_PLANE + kh * S7_IP + j, 0};
    }
    if (s < 72) {
        const int ci = (s - 63) / 3, kh = 2 * ((s - 63) % 3);
        return {(kh * 7 + 6) * 3 + ci, ((kh + 1) * 7 + 6) * 3 + ci, ci * S7_PLANE + kh * S7_IP + 3, 1};
    }
    if (s == 72) return {48 * 3, 48 * 3 + 1, 6 * S7_IP + 3, 2};
    return {48 * 3 + 2, -1, 2 * S7_PLANE + 6 * S7_IP + 3, 0};
}

__device__ __forceinline__ float s7_nanmax(float m, float v) { return (v > m || v != v) ? v : m; }   // torch max_pool2d: a NaN wins and stays

__global__ __launch_bounds__(256, 2) void stem7_pool_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ y, int y_cs, int y_co, int H, int W,
                                                        int Hc, int Wc, int Hp, int Wp, int tiles_h, int tiles_w, long tiles) {
    __shared__ float s_in[3 * S7_PLANE];
    __shared__ __attribute__((aligned(16))) float s_out[128 * S7_OP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hh = lane >> 5;
    // B[k][cout]: lane = cout (li) and the step's first / second tap (hh)
    float b[S7_KS][2];
#pragma unroll
    for (int s = 0; s < S7_KS; ++s) {
        const int k = hh ? s7_step(s).k1 : s7_step(s).k0;
        b[s][0] = k >= 0 ? w[k * 64 + li] : 0.f;
        b[s][1] = k >= 0 ? w[k * 64 + 32 + li] : 0.f;
    }
    const float sc0 = scale[li], sc1 = scale[32 + li], sh0 = shift[li], sh1 = shift[32 + li];
    // this lane's GEMM row: conv pixel (pr, pc) of the tile; the 11 idle rows read pixel 0
    const int p = wave * 32 + li;
    const int pq = p < S7_CPIX ? p : 0;
    const int base = 2 * (pq / S7_CC) * S7_IP + pq % S7_CC;
    const int base_d[3] = {base + hh * S7_HALF, base + hh * S7_IP, base + hh * S7_PLANE};   // the second tap of a step: next column / row / channel
    const float ninf = -__builtin_inff();

    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int tw = (int)(tile % tiles_w);
        const long tr = tile / tiles_w;
        const int th = (int)(tr % tiles_h);
        const int n = (int)(tr / tiles_h);
        const int ph0 = th * S7_PH, pw0 = tw * S7_PW;
        const int ch0 = 2 * ph0 - 1, cw0 = 2 * pw0 - 1;      // conv pixel of tile row / column 0
        const int ih0 = 2 * ch0 - 3, iw0 = 2 * cw0 - 3;      // input pixel of patch row / column 0
        __syncthreads();                                     // the previous tile's pooling has read s_out
        // 1. input patch
        const float* xn = x + (long)n * 3 * H * W;
        for (int i = tid; i < 3 * S7_IR * S7_IC; i += 256) {
            const int c = i % S7_IC, rr = i / S7_IC;
            const int r = rr % S7_IR, ci = rr / S7_IR;
            const int ih = ih0 + r, iw = iw0 + c;
            float v = 0.f;
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = xn[((long)ci * H + ih) * W + iw];
            s_in[ci * S7_PLANE + r * S7_IP + (c & 1) * S7_HALF + (c >> 1)] = v;
        }
        __syncthreads();
        // 2. conv + BN + ReLU into LDS
        s7_f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < S7_KS; ++s) {
            float a = s_in[base_d[s7_step(s).kind] + s7_step(s).off];
            if (s == S7_KS - 1 && hh) a = 0.f;               // the 148th tap does not exist
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[s][0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[s][1], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;     // accumulator row -> conv pixel of the tile
            const int ch = ch0 + q / S7_CC, cw = cw0 + q % S7_CC;
            const bool in_map = q < S7_CPIX && ch >= 0 && ch < Hc && cw >= 0 && cw < Wc;
            float v0 = acc0[r] * sc0 + sh0, v1 = acc1[r] * sc1 + sh1;
            v0 = v0 < 0.f ? 0.f : v0;                        // relu that keeps a NaN
            v1 = v1 < 0.f ? 0.f : v1;
            s_out[q * S7_OP + li] = in_map ? v0 : ninf;
            s_out[q * S7_OP + 32 + li] = in_map ? v1 : ninf;
        }
        __syncthreads();
        // 3. 3x3 stride-2 max, float4 per thread
        for (int i = tid; i < S7_PH * S7_PW * 16; i += 256) {
            const int c4 = i & 15, pp = i >> 4;
            const int pr = pp / S7_PW, pc = pp % S7_PW;
            const int ph = ph0 + pr, pw = pw0 + pc;
            if (ph >= Hp || pw >= Wp) continue;
            s7_f32x4 m = {ninf, ninf, ninf, ninf};
#pragma unroll
            for (int dr = 0; dr < 3; ++dr)
#pragma unroll
                for (int dc = 0; dc < 3; ++dc) {
                    const s7_f32x4 v = *reinterpret_cast<const s7_f32x4*>(&s_out[((2 * pr + dr) * S7_CC + 2 * pc + dc) * S7_OP + c4 * 4]);
                    m[0] = s7_nanmax(m[0], v[0]); m[1] = s7_nanmax(m[1], v[1]); m[2] = s7_nanmax(m[2], v[2]); m[3] = s7_nanmax(m[3], v[3]);
                }
            *reinterpret_cast<s7_f32x4*>(y + (((long)n * Hp + ph) * Wp + pw) * y_cs + y_co + c4 * 4) = m;
        }
    }
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_stem7x7_bn_relu_maxpool_nchw3(const float* x, const float* w, const float* scale, const float* shift, float* y, int y_cs, int y_co,
                                                 int N, int H, int W, int Cout, void* stream) {
    if (!x || !w || !scale || !shift || !y) return fail(CMK_EINVAL, "stem7: null pointer%s", "");
    if (Cout != 64) return fail(CMK_EINVAL, "stem7: %sCout = %ld must be 64", "", (long)Cout);
    if (N < 1 || H < 1 || W < 1) return fail(CMK_EINVAL, "stem7: empty input%s (N = %ld, H x W = %ld; all must be >= 1)", "", (long)N, (long)H * W);
    if ((y_cs & 3) || (y_co & 3) || y_co < 0 || (long)y_co + Cout > y_cs)
        return fail(CMK_EINVAL, "stem7: %soutput view: pixel stride %ld and channel offset %ld must be multiples of 4 floats with offset + 64 <= stride", "",
                    (long)y_cs, (long)y_co);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)scale | (uintptr_t)shift) & 3 || ((uintptr_t)y & 15))
        return fail(CMK_EINVAL, "stem7: x, w, scale, shift must be 4-byte and y 16-byte aligned%s", "");
    if ((long)3 * H * W >= (1L << 31)) return fail(CMK_EINVAL, "stem7: image too large%s (3 * H * W = %ld must be below 2^31)", "", (long)3 * H * W);
    const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1;
    const int Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;
    const int tiles_h = cdiv(Hp, S7_PH), tiles_w = cdiv(Wp, S7_PW);
    const long tiles = (long)N * tiles_h * tiles_w;      // every global offset in the kernel is 64-bit
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    hipLaunchKernelGGL(stem7_pool_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift, y, y_cs, y_co, H, W, Hc, Wc, Hp, Wp, tiles_h,
                       tiles_w, tiles);
    return check_launch("stem7_pool");
}
