// Deformable 3x3 conv (d2 DeformConv / ModulatedDeformConv, stride 1, pad 1, dilation 1, groups 1, no bias) as an implicit
// GEMM on v_mfma_f32_32x32x2_f32, with the FrozenBN fold and ReLU of DFConv3x3 in the epilogue.
//
//   GEMM view:  M = output pixels (flattened N*H*W), N = output channels, K = 9 taps x Cin, all fp32 — the GA (gather) form of
//   conv_igemm.hip with a bilinearly sampled A operand instead of a shifted halo.
//   Block = 4 waves stacked along M, 32 pixels each (128 pixels per workgroup); every wave holds WN <= 7 accumulators of 32x32,
//   so one workgroup covers the whole layer width (the DCN layers' Cout is the stage width, 64..224) and every sampled value
//   feeds each output channel exactly once.
//   K is walked tap-major: at the start of tap t the workgroup computes, once per (pixel, deformable group), the four corner
//   pixel indices and the four bilinear weights (mask = sigmoid(logit) folded in) into LDS; every 16-channel chunk of that tap
//   then reads them back.  A corner that must not be read (it lies outside the map, its sample lies outside (-1,H) x (-1,W), or
//   its pixel is past the last one) gets the index -1: load_A skips its load (the lane is masked off) and blends a zero quad, so
//   nothing is multiplied by 0 and no Inf or NaN of a stand-in address can reach the output.  An in-map corner of weight 0 is
//   read and multiplied, as the float64 restatement does.  In NHWC a corner is a contiguous run of
//   channels, so a thread gathers its 4 channels of a pixel as four 16-byte loads and blends them with three FMAs + one mul.
//   K order inside a 16-chunk is that of conv_igemm.hip (MFMA k-step s of lane half h uses channel 8h+s); a lane half's 8
//   channels lie in one deformable group whenever (Cin/dg) % 8 == 0, which the host checks.
//   Weights: the conv_igemm.hip packing [tap][Cin/16][cout_pad][16] (cmk_conv_packed_floats(Cout, Cin, 3)).
//   Pipeline: register-staged double buffering of the A/B slabs within a tap (one barrier per chunk), two barriers per tap
//   around the sample-table pass.
//
// Reference call site replaced: DFConv3x3.forward (vovnet.py:185-201): conv_offset's output split (chunk/cat, sigmoid) and
// d2 DeformConv / ModulatedDeformConv, then FrozenBN + ReLU.
#include "conv_args.hpp"

namespace cmk {

namespace {

constexpr int DBM = 128;      // pixels per workgroup
constexpr int DMAXG = 4;      // deformable groups supported
constexpr int A_FLOATS = DBM * PST;

struct DeformArgs {
    const float* x; int x_cs, x_co;
    const float* off; int off_cs;
    const float* w; const float* scale; const float* shift;
    float* y; int y_cs, y_co;
    int N, H, W, Cin, Cout, dg, cpg, modulated, relu;
    int cout_pad;
    long total_pix;
};

struct __attribute__((aligned(16))) Sample {   // one (pixel, group) of a tap: corner pixel indices (within the batch) + weights
    int o[4];
    float w[4];
};

template <int WN>
struct DGeo {
    static constexpr int BN = 32 * WN;
    static constexpr int B_FLOATS = BN * PST;
    static constexpr int B_ITERS = (BN * 4 + 255) / 256;
    static constexpr int LDS_BYTES = (2 * A_FLOATS + 2 * B_FLOATS) * 4 + DBM * DMAXG * (int)sizeof(Sample);
};

template <int WN>
__global__ __launch_bounds__(256, 2) void conv_deform_kernel(const DeformArgs a) {
    using G = DGeo<WN>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;
    float* sB = smem + 2 * A_FLOATS;
    Sample* sS = reinterpret_cast<Sample*>(smem + 2 * A_FLOATS + 2 * G::B_FLOATS);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hh = lane >> 5;
    const int li = lane & 31;
    const long pix0 = (long)blockIdx.x * DBM;
    const int co0 = blockIdx.y * G::BN;
    const int H = a.H, W = a.W, dg = a.dg;
    const long hw = (long)H * W;
    const int cin_chunks = a.Cin >> 4;

    // ---- sample table of one tap: (pixel, group) items, at most 2 per thread --------------------------------------------
    auto make_samples = [&](int tap) {
        const int ki = tap / 3, kj = tap - ki * 3;
        for (int item = tid; item < DBM * dg; item += 256) {
            const int p = item / dg, g = item - p * dg;
            const long P = pix0 + p;
            Sample s;
            s.o[0] = s.o[1] = s.o[2] = s.o[3] = -1;          // -1: nothing is read for this corner
            s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
            if (P < a.total_pix) {
                const int n = (int)(P / hw);
                const int rem = (int)(P - (long)n * hw);
                const int h = rem / W, w = rem - h * W;
                const float* op = a.off + P * a.off_cs;
                const float dy = op[g * 18 + 2 * tap], dx = op[g * 18 + 2 * tap + 1];
                float m = 1.f;
                if (a.modulated) m = 1.f / (1.f + expf(-op[18 * dg + g * 9 + tap]));
                const float py = (float)(h - 1 + ki) + dy, px = (float)(w - 1 + kj) + dx;
                const int base = n * H * W;
                if (py > -1.f && px > -1.f && py < (float)H && px < (float)W) {
                    const float fy = floorf(py), fx = floorf(px);
                    const int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
                    const float ly = py - fy, lx = px - fx, uy = 1.f - ly, ux = 1.f - lx;
                    const bool vy0 = y0 >= 0, vy1 = y1 <= H - 1, vx0 = x0 >= 0, vx1 = x1 <= W - 1;
                    if (vy0 && vx0) { s.o[0] = base + y0 * W + x0; s.w[0] = uy * ux * m; }
                    if (vy0 && vx1) { s.o[1] = base + y0 * W + x1; s.w[1] = uy * lx * m; }
                    if (vy1 && vx0) { s.o[2] = base + y1 * W + x0; s.w[2] = ly * ux * m; }
                    if (vy1 && vx1) { s.o[3] = base + y1 * W + x1; s.w[3] = ly * lx * m; }
                }
            }
            sS[item] = s;
        }
    };

    // ---- A: 128 pixels x 16 channels of one chunk, 2 (pixel, channel quad) items per thread -----------------------------
    const float* xin = a.x + a.x_co;
    f32x4 a_stage[2];
    auto load_A = [&](int chunk) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = it * 256 + tid;
            const int p = idx >> 2, q = idx & 3;
            const int ch = chunk * 16 + q * 4;
            const int g = ch / a.cpg;
            const Sample s = sS[p * dg + g];
            const float* src = xin + ch;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {               // a predicated load: an unread corner is a zero quad, not a product with 0
                v[k] = zero;
                if (s.o[k] >= 0) v[k] = *reinterpret_cast<const f32x4*>(src + (long)s.o[k] * a.x_cs);
            }
            a_stage[it] = v[0] * s.w[0] + v[1] * s.w[1] + v[2] * s.w[2] + v[3] * s.w[3];
        }
    };
    auto store_A = [&](int buf) {
        float* dst = sA + buf * A_FLOATS;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = it * 256 + tid;
            *reinterpret_cast<f32x4*>(dst + (idx >> 2) * PST + (idx & 3) * 4) = a_stage[it];
        }
    };
    // ---- B: [BN couts][16 ci] slab of the packed weights ---------------------------------------------------------------
    f32x4 b_stage[G::B_ITERS];
    auto load_B = [&](int tap, int chunk) {
        const float* wsrc = a.w + (long)(tap * cin_chunks + chunk) * a.cout_pad * 16;
#pragma unroll
        for (int it = 0; it < G::B_ITERS; ++it) {
            int idx = it * 256 + tid;
            if ((it + 1) * 256 > G::BN * 4) idx = min(idx, G::BN * 4 - 1);
            const int row = min(co0 + (idx >> 2), a.cout_pad - 1);     // rows past cout_pad (last tile) feed discarded columns
            b_stage[it] = *reinterpret_cast<const f32x4*>(wsrc + row * 16 + (idx & 3) * 4);
        }
    };
    auto store_B = [&](int buf) {
        float* dst = sB + buf * G::B_FLOATS;
#pragma unroll
        for (int it = 0; it < G::B_ITERS; ++it) {
            const int idx = it * 256 + tid;
            if ((it + 1) * 256 <= G::BN * 4 || idx < G::BN * 4)
                *reinterpret_cast<f32x4*>(dst + (idx >> 2) * PST + (idx & 3) * 4) = b_stage[it];
        }
    };

    const int a_off = (wave * 32 + li) * PST + hh * 8;
    const int b_off = li * PST + hh * 8;
    f32x16 acc[WN];
#pragma unroll
    for (int nn = 0; nn < WN; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nn][r] = 0.f;

#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        __syncthreads();              // every wave is done with the previous tap's samples and slabs
        make_samples(tap);
        __syncthreads();
        load_A(0);
        load_B(tap, 0);
        store_A(0);
        store_B(0);
#pragma unroll 1
        for (int c = 0; c < cin_chunks; ++c) {
            const bool has_next = c + 1 < cin_chunks;
            if (has_next) {
                load_A(c + 1);
                load_B(tap, c + 1);
            }
            __syncthreads();          // slabs of chunk c visible; every wave is done with chunk c-1
            const float* A = sA + (c & 1) * A_FLOATS + a_off;
            const float* B = sB + (c & 1) * G::B_FLOATS + b_off;
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(A);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(A + 4);
#pragma unroll
            for (int nn = 0; nn < WN; ++nn) {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(B + nn * 32 * PST);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(B + nn * 32 * PST + 4);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc[nn], 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1[s], acc[nn], 0, 0, 0);
            }
            if (has_next) {
                store_A((c + 1) & 1);
                store_B((c + 1) & 1);
            }
        }
    }

    // ---- epilogue: folded FrozenBN (+ReLU) into the output slice ----------------------------------------------------------
#pragma unroll
    for (int nn = 0; nn < WN; ++nn) {
        const int co = co0 + nn * 32 + li;
        if (co >= a.Cout) continue;
        const float sc = a.scale[co], sh = a.shift[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            const long P = pix0 + wave * 32 + row;
            if (P < a.total_pix) {
                float v = acc[nn][r] * sc + sh;
                if (a.relu) v = fmaxf(v, 0.f);
                a.y[P * a.y_cs + a.y_co + co] = v;
            }
        }
    }
}

template <int WN>
int launch_deform(const DeformArgs& a, int ntiles, hipStream_t st) {
    using G = DGeo<WN>;
    static DeviceOnce once;
    int rc = once.run([]() {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_deform_kernel<WN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           G::LDS_BYTES);
        return e == hipSuccess ? CMK_OK : fail(CMK_ELAUNCH, "deform_conv: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    });
    if (rc) return rc;
    const long blocks = (a.total_pix + DBM - 1) / DBM;
    hipLaunchKernelGGL(conv_deform_kernel<WN>, dim3((unsigned)blocks, ntiles), dim3(256), G::LDS_BYTES, st, a);
    return check_launch("deform_conv");
}

}  // namespace
}  // namespace cmk

extern "C" int cmk_deform_conv3x3_nhwc(const float* x, int x_cs, int x_co, const float* offsets, int off_cs, const float* w,
                                       const float* scale, const float* shift, float* y, int y_cs, int y_co, int N, int H, int W,
                                       int Cin, int Cout, int dg, int modulated, int relu, void* stream) {
    using namespace cmk;
    if (!x || !offsets || !w || !scale || !shift || !y) return fail(CMK_EINVAL, "deform_conv: null pointer%s", "");
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return fail(CMK_EINVAL, "deform_conv: empty shape%s", "");
    if ((x_cs & 3) || (x_co & 3) || x_co < 0 || (long)x_co + Cin > x_cs || ((uintptr_t)x & 15))
        return fail(CMK_EINVAL, "deform_conv: input view must be 16-byte aligned (stride and offset multiples of 4) and hold Cin channels%s", "");
    if ((uintptr_t)w & 15) return fail(CMK_EINVAL, "deform_conv: the packed weights are read as 16-byte vectors, w must be 16-byte aligned%s", "");
    if (((uintptr_t)offsets | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)y) & 3)
        return fail(CMK_EINVAL, "deform_conv: offsets, scale, shift and y must be 4-byte aligned%s", "");
    if (y_co < 0 || (long)y_co + Cout > y_cs) return fail(CMK_EINVAL, "deform_conv: output view (%s%ld channels) does not hold Cout", "", (long)y_cs);
    if (x == y && x_co < y_co + Cout && y_co < x_co + Cin)
        return fail(CMK_EINVAL, "deform_conv: input and output channel slices of one buffer overlap%s", "");
    if (dg < 1 || Cin % dg) return fail(CMK_EINVAL, "deform_conv: deformable groups (%s%ld) do not divide Cin", "", (long)dg);
    if (dg != 1 && dg != 2 && dg != 4) return fail(CMK_EINVAL, "deform_conv: deformable groups %s%ld not supported (1, 2 or 4)", "", (long)dg);
    if ((Cin / dg) % 8) return fail(CMK_EINVAL, "deform_conv: Cin/dg = %s%ld is not a multiple of 8", "", (long)(Cin / dg));
    if (Cin % 16) return fail(CMK_EINVAL, "deform_conv: Cin (%s%ld) must be a multiple of 16", "", (long)Cin);
    const int need = (modulated ? 27 : 18) * dg;
    if (off_cs < need) return fail(CMK_EINVAL, "deform_conv: offset tensor has %s%ld channels, needs %ld", "", (long)off_cs, (long)need);
    const long total_pix = (long)N * H * W;
    if (total_pix * (long)(x_cs > y_cs ? x_cs : y_cs) >= (1L << 31) || total_pix * off_cs >= (1L << 31))
        return fail(CMK_EINVAL, "deform_conv: tensor too large%s", "");
    DeformArgs a;
    a.x = x; a.x_cs = x_cs; a.x_co = x_co;
    a.off = offsets; a.off_cs = off_cs;
    a.w = w; a.scale = scale; a.shift = shift;
    a.y = y; a.y_cs = y_cs; a.y_co = y_co;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.dg = dg; a.cpg = Cin / dg; a.modulated = modulated ? 1 : 0; a.relu = relu ? 1 : 0;
    a.cout_pad = cmk_conv_cout_pad(Cout);
    a.total_pix = total_pix;
    const int c32 = (Cout + 31) / 32;
    const int ntiles = (c32 + 6) / 7;                 // cout tiles of at most 224 channels, as even as possible
    const int wn = (c32 + ntiles - 1) / ntiles;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (wn) {
        case 1: return launch_deform<1>(a, ntiles, st);
        case 2: return launch_deform<2>(a, ntiles, st);
        case 3: return launch_deform<3>(a, ntiles, st);
        case 4: return launch_deform<4>(a, ntiles, st);
        case 5: return launch_deform<5>(a, ntiles, st);
        case 6: return launch_deform<6>(a, ntiles, st);
        default: return launch_deform<7>(a, ntiles, st);
    }
}
