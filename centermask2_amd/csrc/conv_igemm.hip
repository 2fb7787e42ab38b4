// Convolution (3x3 s1/s2, 1x1, and FC as 1x1 over "pixels" = rows) as an implicit GEMM on the CDNA4 matrix pipe.
//
//   GEMM view:  M = output pixels, N = output channels, K = taps * Cin, all fp32.
//   Instruction: v_mfma_f32_32x32x2_f32 — exact fp32 (bitwise a k-ordered fmaf chain), 64 FLOP/clk/SIMD, the same
//   peak as the fp32 VALU but one VGPR per operand, so the tile is fed from LDS with ds_read_b128 instead of
//   per-FMA register traffic.  A 32x32 accumulator's column sits on the lane, so Cout is mapped to the lane
//   (128-byte contiguous NHWC stores) and pixels to the accumulator rows.
//
//   Tiling (block = 4 waves stacked along M, wave tile = WM x WN accumulators of 32 pixels x 32 couts):
//     3x3:  spatial tile of (4*WM*SR) x SC output pixels, a wave sub-tile being SR x SC = 2x16 or 1x32 pixels; the
//           input halo tile is staged ONCE per 16-channel K chunk in LDS and the 9 taps read it at shifted addresses
//           (9x fewer global->LDS bytes than per-tap im2col).
//     1x1:  128*WM consecutive pixels of the flattened (N*H*W) axis.
//     Per K chunk and tap the block stages a [32*WN couts][16 ci] weight slab (pre-packed, contiguous in HBM).
//   K order inside a 16-chunk is permuted so that MFMA k-step s of lane half h uses channel 8h+s: every lane then
//   reads 8 contiguous floats per operand row (2 x ds_read_b128) for 8 MFMAs.  Rows are padded to 20 floats
//   (80 B), which spreads the 16-lane ds_read_b128 groups over all 16-byte LDS slots.
//   Pipeline: global loads for step s+1 (weights) and chunk c+1 (halo) are issued before the barrier of step s
//   and written to the other LDS buffer after its MFMAs (register-staged double buffering, one barrier per step).
//   Staging loads are branch-free (clamped address, zero selected at the LDS write) so the compiler keeps them in
//   flight across the MFMA block.
//   Scheduling: the matrix pipe is the bound, so what matters is that every CU holds the same number of equally long
//   workgroups.  The host picks (WM, sub-tile shape) per layer from a small menu with a residency/round cost model
//   (choose_variant), and layers that share weights across FPN levels (FCOS towers/predictors) run as ONE launch
//   whose block index walks the tiles of all levels.
//
// Reference call sites replaced: aten::conv2d + FrozenBN + ReLU vovnet.py:205-236; d2 FPN convs (vovnet.py:547-554);
// fpn.py:27-35; fcos.py:169-200; sam.py:58-83; maskiou_head.py:81-93; nn.Linear maskiou_head.py:89-91.
#include "conv_args.hpp"

namespace cmk {

template <int TAPS, int STRIDE, int WM, int WN, int SC>
struct Geo {
    static constexpr int SR = 32 / SC;   // sub-tile rows
    static constexpr int SUBT = 4 * WM;  // 32-pixel sub-tiles per block
    static constexpr int BM = 32 * SUBT;
    static constexpr int BN = 32 * WN;
    static constexpr int TH = (TAPS == 9) ? SR * SUBT : 1;
    static constexpr int TW = (TAPS == 9) ? SC : BM;
    static constexpr int HH = (TAPS == 9) ? (TH - 1) * STRIDE + 3 : 1;
    static constexpr int HWD = (TAPS == 9) ? (TW - 1) * STRIDE + 3 : BM;
    static constexpr int APIX = HH * HWD;
    static constexpr int A_BYTES = APIX * PST * 4;
    static constexpr int B_BYTES = BN * PST * 4;
    static constexpr int OCC = occ_of(WM, WN, STRIDE);
    static constexpr bool ADB = (2 * A_BYTES + 2 * B_BYTES) * OCC <= LDS_CU;   // double-buffer the halo only if residency is kept
    static constexpr int LDS_BYTES = (ADB ? 2 : 1) * A_BYTES + 2 * B_BYTES;
    static constexpr int RESIDENT = (LDS_BYTES * OCC <= LDS_CU) ? OCC : (LDS_BYTES * 2 <= LDS_CU ? 2 : 1);
    static constexpr int A_ITERS = (APIX * 4 + 255) / 256;
    static constexpr int B_ITERS = (BN * 4 + 255) / 256;
};

// GA ("gather") form: a 3x3 conv run as a flattened-pixel GEMM (TAPS == 1 geometry) whose K walks 9 taps x Cin/16 chunks; each
// thread gathers its A rows per tap straight from the image (zero outside).  No halo reuse, so it only pays on maps too small
// to fill the spatial tiles (7x7 RoI maps, P6/P7).
template <int TAPS, int STRIDE, int WM, int WN, int SC, bool GA = false>
__global__ __launch_bounds__(256, (occ_of(WM, WN, STRIDE))) void conv_igemm_kernel(const ConvArgs a) {
    using G = Geo<TAPS, STRIDE, WM, WN, SC>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;
    float* sB = smem + (G::ADB ? 2 : 1) * G::APIX * PST;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hh = lane >> 5;  // k half
    const int li = lane & 31;

    // ---- which problem (FPN level) and which tile ------------------------------------------------------------
    // XCD-aware order (see conv_wino4r_kernel): the grid_y workgroups of one input tile go to one XCD, back to back
    const int xq = blockIdx.x >> 3, xcd = blockIdx.x & 7;
    const int bx = (xq / a.grid_y) * 8 + xcd, by = xq % a.grid_y;
    if (bx >= a.total_tiles) return;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAXP; ++i)
        if (i < a.nprob && bx >= a.p[i].tile_begin) pi = i;
    const ConvProblem& P = a.p[pi];
    const int H = P.H, W = P.W, Ho = P.Ho, Wo = P.Wo;
    const long total_pix = P.total_pix;
    const int tile = bx - P.tile_begin;
    int n = 0, oh0 = 0, ow0 = 0;
    long pix0 = 0;
    if (TAPS == 9) {
        int tw = tile % P.tiles_w;
        int t2 = tile / P.tiles_w;
        int th = t2 % P.tiles_h;
        n = t2 / P.tiles_h;
        oh0 = th * G::TH;
        ow0 = tw * G::TW;
    } else {
        pix0 = (long)tile * G::BM;
    }
    const int co0 = by * G::BN;
    const int cin_chunks = a.Cin >> 4;
    const int nchunks = GA ? 9 * cin_chunks : cin_chunks;
    const int c_lo = (int)((long)blockIdx.y * nchunks / a.ksplit), c_hi = (int)((long)(blockIdx.y + 1) * nchunks / a.ksplit);  // even bounds (host)
    const int total_steps = c_hi * TAPS;

    // ---- per-thread staging descriptors ------------------------------------------------------------------------
    const float* xin = P.x + (TAPS == 9 ? (long)n * H * W * a.x_cs : 0L) + a.x_co;
    long a_goff[G::A_ITERS];   // clamped to a valid address; a_ok tells whether the value is used
    int ga_ih0[GA ? G::A_ITERS : 1], ga_iw0[GA ? G::A_ITERS : 1];   // GA: top-left input coordinate of the row's 3x3 window
    unsigned a_ok = 0;
#pragma unroll
    for (int it = 0; it < G::A_ITERS; ++it) {
        int idx = it * 256 + tid;
        int pix = idx >> 2, q = idx & 3;
        long off = 0;
        if (idx < G::APIX * 4) {
            if (GA) {
                long Pp = pix0 + pix;
                const bool pv = Pp < total_pix;
                if (!pv) Pp = 0;
                const long hw = (long)Ho * Wo;
                const int n_ = (int)(Pp / hw);
                const int rem = (int)(Pp - (long)n_ * hw);
                const int oh = rem / Wo, ow = rem - oh * Wo;
                ga_ih0[it] = pv ? oh * a.ga_stride - 1 : -4;      // -4: every tap lands outside
                ga_iw0[it] = ow * a.ga_stride - 1;
                off = (long)n_ * H * W * a.x_cs + q * 4;
            } else if (TAPS == 9) {
                int hr = pix / G::HWD, hc = pix - hr * G::HWD;
                int ih = oh0 * STRIDE - 1 + hr, iw = ow0 * STRIDE - 1 + hc;
                if (ih >= 0 && ih < H && iw >= 0 && iw < W) { off = ((long)ih * W + iw) * a.x_cs + q * 4; a_ok |= 1u << it; }
            } else {
                long Pp = pix0 + pix;
                if (Pp < total_pix) { off = Pp * a.x_cs + q * 4; a_ok |= 1u << it; }
            }
        }
        a_goff[it] = off;
    }
    f32x4 a_stage[G::A_ITERS];
    f32x4 b_stage[G::B_ITERS];
    // fused input affine (GroupNorm apply + ReLU of the producer): the channel quad of a thread is fixed (idx & 3 == tid & 3)
    const bool has_aff = P.in_scale != nullptr;
    int aff_n = n;                                   // 1x1 (flattened pixels): image index of this tile's first pixel; tiles never
    if (TAPS != 9 && has_aff) aff_n = (int)(pix0 / ((long)Ho * Wo));   // straddle images when the affine is used (checked on the host)
    const float* aff_s = has_aff ? P.in_scale + (long)aff_n * a.Cin + (tid & 3) * 4 : nullptr;
    const float* aff_b = has_aff ? P.in_shift + (long)aff_n * a.Cin + (tid & 3) * 4 : nullptr;
    f32x4 in_sc = {1.f, 1.f, 1.f, 1.f}, in_sh = {0.f, 0.f, 0.f, 0.f};

    auto load_A = [&](int chunk) {
        if (GA) {
            const int tap = chunk / cin_chunks, ch = chunk - tap * cin_chunks;
            const int kh = tap / 3, kw = tap - kh * 3;
            a_ok = 0;
#pragma unroll
            for (int it = 0; it < G::A_ITERS; ++it) {
                const int ih = ga_ih0[it] + kh, iw = ga_iw0[it] + kw;
                const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
                const long off = ok ? a_goff[it] + ((long)ih * W + iw) * a.x_cs + ch * 16 : 0L;
                a_stage[it] = *reinterpret_cast<const f32x4*>(xin + off);
                a_ok |= (ok ? 1u : 0u) << it;
            }
            return;
        }
#pragma unroll
        for (int it = 0; it < G::A_ITERS; ++it) a_stage[it] = *reinterpret_cast<const f32x4*>(xin + a_goff[it] + chunk * 16);
        if (has_aff) {
            in_sc = *reinterpret_cast<const f32x4*>(aff_s + chunk * 16);
            in_sh = *reinterpret_cast<const f32x4*>(aff_b + chunk * 16);
        }
    };
    auto store_A = [&](int buf) {
        float* dst = sA + buf * (G::APIX * PST);
#pragma unroll
        for (int it = 0; it < G::A_ITERS; ++it) {
            int idx = it * 256 + tid;
            if ((it + 1) * 256 <= G::APIX * 4 || idx < G::APIX * 4) {
                f32x4 v = a_stage[it];
                const bool ok = (a_ok >> it) & 1u;
                // rare, wave-uniform options: real branches (the empty asm keeps hipcc from if-converting them into selects that
                // every conv would execute — each VALU instruction here costs the matrix pipe ~4 cycles, tools/probe/mfma_probe2.hip)
                if (has_aff) {
                    asm volatile("" ::: "memory");
                    v.x = fmaxf(v.x * in_sc.x + in_sh.x, 0.f); v.y = fmaxf(v.y * in_sc.y + in_sh.y, 0.f);
                    v.z = fmaxf(v.z * in_sc.z + in_sh.z, 0.f); v.w = fmaxf(v.w * in_sc.w + in_sh.w, 0.f);
                }
                if (a.in_relu) {
                    asm volatile("" ::: "memory");
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                v.x = ok ? v.x : 0.f;
                v.y = ok ? v.y : 0.f;
                v.z = ok ? v.z : 0.f;
                v.w = ok ? v.w : 0.f;
                *reinterpret_cast<f32x4*>(dst + (idx >> 2) * PST + (idx & 3) * 4) = v;
            }
        }
    };
    auto load_B = [&](int step) {
        int chunk = step / TAPS, tap = step - chunk * TAPS;
        const float* wsrc = a.w + ((long)(tap * nchunks + chunk) * a.cout_pad + co0) * 16;
#pragma unroll
        for (int it = 0; it < G::B_ITERS; ++it) {
            int idx = it * 256 + tid;
            if ((it + 1) * 256 > G::BN * 4) idx = min(idx, G::BN * 4 - 1);   // ragged last iteration: clamp, do not branch
            b_stage[it] = *reinterpret_cast<const f32x4*>(wsrc + idx * 4);
        }
    };
    auto store_B = [&](int buf) {
        float* dst = sB + buf * (G::BN * PST);
#pragma unroll
        for (int it = 0; it < G::B_ITERS; ++it) {
            int idx = it * 256 + tid;
            if ((it + 1) * 256 <= G::BN * 4 || idx < G::BN * 4)
                *reinterpret_cast<f32x4*>(dst + (idx >> 2) * PST + (idx & 3) * 4) = b_stage[it];
        }
    };

    // ---- MFMA operand addresses -----------------------------------------------------------------------------------
    int a_off[WM];
#pragma unroll
    for (int m = 0; m < WM; ++m) {
        int u = wave * WM + m;
        if (TAPS == 9) {
            int r = li / SC, cc = li % SC;
            a_off[m] = (((u * G::SR + r) * STRIDE) * G::HWD + cc * STRIDE) * PST + hh * 8;
        } else {
            a_off[m] = (u * 32 + li) * PST + hh * 8;
        }
    }
    const int b_off = li * PST + hh * 8;

    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int nn = 0; nn < WN; ++nn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][nn][r] = 0.f;

    // ---- prologue ---------------------------------------------------------------------------------------------------
    load_A(c_lo);
    load_B(c_lo * TAPS);
    store_A(0);          // c_lo is even, so buffer parity (c & 1, step & 1) starts at 0
    store_B(0);

    int step = c_lo * TAPS;
    for (int c = c_lo; c < c_hi; ++c) {
        const bool has_next_chunk = (c + 1 < c_hi);
        if (has_next_chunk) load_A(c + 1);
        const float* Abase = sA + (G::ADB ? (c & 1) : 0) * (G::APIX * PST);
#pragma unroll 1
        for (int t = 0; t < TAPS; ++t, ++step) {
            const bool has_next = (step + 1 < total_steps);
            if (has_next) load_B(step + 1);
            __syncthreads();  // staged data of this step visible; every wave is done with step-1

            int tapoff = 0;
            if (TAPS == 9) {
                int kh = t / 3, kw = t - kh * 3;
                tapoff = (kh * G::HWD + kw) * PST;
            }
            const float* A = Abase + tapoff;
            const float* B = sB + (step & 1) * (G::BN * PST) + b_off;
            f32x4 a0[WM], a1[WM];
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                a0[m] = *reinterpret_cast<const f32x4*>(A + a_off[m]);
                a1[m] = *reinterpret_cast<const f32x4*>(A + a_off[m] + 4);
            }
#pragma unroll
            for (int nn = 0; nn < WN; ++nn) {
                f32x4 b0 = *reinterpret_cast<const f32x4*>(B + nn * 32 * PST);
                f32x4 b1 = *reinterpret_cast<const f32x4*>(B + nn * 32 * PST + 4);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int m = 0; m < WM; ++m)
                        acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m][s], b0[s], acc[m][nn], 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int m = 0; m < WM; ++m)
                        acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m][s], b1[s], acc[m][nn], 0, 0, 0);
            }
            if (has_next) store_B((step + 1) & 1);
            if (t == TAPS - 1 && has_next_chunk) {
                if (!G::ADB) __syncthreads();  // single halo buffer: everyone must be done reading it
                store_A(G::ADB ? ((c + 1) & 1) : 0);
            }
        }
    }

    // ---- split-K: raw partial sums to the workspace, the reduce kernel applies the epilogue ----------------------------
    if (a.ksplit > 1) {
        float* wz = a.ws + (long)blockIdx.y * total_pix * a.cout_pad + co0 + li;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
            const int u = wave * WM + m;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                long opix;
                bool pvalid;
                if (TAPS == 9) {
                    const int oh = oh0 + u * G::SR + row / SC, ow = ow0 + row % SC;
                    pvalid = (oh < Ho) && (ow < Wo);
                    opix = ((long)n * Ho + oh) * Wo + ow;
                } else {
                    opix = pix0 + u * 32 + row;
                    pvalid = opix < total_pix;
                }
                if (pvalid) {
#pragma unroll
                    for (int nn = 0; nn < WN; ++nn) wz[opix * a.cout_pad + nn * 32] = acc[m][nn][r];
                }
            }
        }
        return;
    }

    // ---- epilogue: scale/shift (+residual) (+ReLU), NHWC store -------------------------------------------------------
#pragma unroll
    for (int nn = 0; nn < WN; ++nn) {
        const int co = co0 + nn * 32 + li;
        const bool cvalid = co < a.Cout;
        const float sc = cvalid ? P.scale[co] : 0.f;
        const float sh = cvalid ? P.shift[co] : 0.f;
        const bool do_relu = co < a.relu_upto;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
            const int u = wave * WM + m;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                long opix;
                bool pvalid;
                int oh = 0, ow = 0;
                if (TAPS == 9) {
                    oh = oh0 + u * G::SR + row / SC;
                    ow = ow0 + row % SC;
                    pvalid = (oh < Ho) && (ow < Wo);
                    opix = ((long)n * Ho + oh) * Wo + ow;
                } else {
                    opix = pix0 + u * 32 + row;
                    pvalid = opix < total_pix;
                }
                if (cvalid && pvalid) {
                    float v = acc[m][nn][r] * sc + sh;
                    if (a.res_mode == 1) {
                        v += a.res[opix * a.res_cs + a.res_co + co];
                    } else if (a.res_mode == 2) {
                        int nn_ = n;
                        if (TAPS != 9) {  // recover (n, oh, ow) from the flattened pixel index
                            long hw = (long)Ho * Wo;
                            nn_ = (int)(opix / hw);
                            int rem = (int)(opix - (long)nn_ * hw);
                            oh = rem / Wo;
                            ow = rem - oh * Wo;
                        }
                        long rp = ((long)nn_ * a.Hr + (oh >> 1)) * a.Wr + (ow >> 1);
                        v += a.res[rp * a.res_cs + a.res_co + co];
                    }
                    if (do_relu) v = fmaxf(v, 0.f);
                    P.y[opix * a.y_cs + a.y_co + co] = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side: variant menu + cost model
// ---------------------------------------------------------------------------------------------------------------
template <int TAPS, int STRIDE, int WM, int WN, int SC, bool GA = false>
static int launch(ConvArgs& a, int grid_y, hipStream_t st, LaunchPlan* plan) {
    using G = Geo<TAPS, STRIDE, WM, WN, SC>;
    static DeviceOnce once;      // one per template instantiation
    auto kern = conv_igemm_kernel<TAPS, STRIDE, WM, WN, SC, GA>;
    int rc0 = plan ? CMK_OK : once.run([kern]() {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
        return e == hipSuccess ? CMK_OK : fail(CMK_ELAUNCH, "conv: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    });
    if (rc0) return rc0;
    int blocks = 0;
    for (int i = 0; i < a.nprob; ++i) {
        ConvProblem& p = a.p[i];
        p.tile_begin = blocks;
        if (TAPS == 9) {
            p.tiles_h = cdiv(p.Ho, G::TH);
            p.tiles_w = cdiv(p.Wo, G::TW);
            blocks += p.N * p.tiles_h * p.tiles_w;
        } else {
            p.tiles_h = p.tiles_w = 0;
            blocks += (int)((p.total_pix + G::BM - 1) / G::BM);
        }
    }
    a.grid_y = grid_y;
    a.total_tiles = blocks;
    if (a.ksplit < 1) a.ksplit = 1;
    const int vchunks = (GA ? 9 : 1) * (a.Cin >> 4);
    if (a.ksplit > 1 && (a.nprob != 1 || a.res_mode == 2 || !a.ws || vchunks % (2 * a.ksplit)))
        return fail(CMK_EINVAL, "conv: split-K needs one problem, a workspace, no upsampled residual and K chunks %% (2*splitk) == 0%s", "");
    if (plan) {      // every block: BM pixels x BN couts over K = taps x Cin (the gather form walks the 9 taps as K chunks)
        snprintf(plan->kernel, sizeof(plan->kernel), "conv_igemm_kernel<%d, %d, %d, %d, %d, %s>", TAPS, STRIDE, WM, WN, SC, tf(GA));
        plan->executed_flops = 2 * (int64_t)blocks * G::BM * grid_y * G::BN * (GA ? 9 : TAPS) * a.Cin;
        return CMK_OK;
    }
    hipLaunchKernelGGL(kern, dim3(((blocks + 7) / 8) * 8 * grid_y, a.ksplit), dim3(256), G::LDS_BYTES, st, a);
    return check_launch("conv_igemm");     // split-K: run() reduces the partial sums
}

// cost of running `blocks` equal workgroups with `resident` per CU on 256 CUs: full rounds keep every CU at `resident`
// workgroups; the last round spreads round-robin.  eff(j) = matrix-pipe utilisation with j workgroups on a CU.
static double round_cost(long blocks, int resident, double wg_cost) {
    static const double eff[4] = {1.0, 0.70, 0.90, 0.95};
    const long slots = 256L * resident;
    long full = blocks / slots, rem = blocks % slots;
    double c = (double)full * resident * wg_cost / eff[resident];
    if (rem) {
        int j = (int)((rem + 255) / 256);
        c += (double)j * wg_cost / eff[j];
    }
    return c;
}

bool variant_ok(int taps, int stride, int cout32, int wm, int sc, int wn) {
    if (wn < 1 || wn > 7 || (wm != 1 && wm != 2) || (sc != 16 && sc != 32)) return false;
    if (cout32 <= 7 ? (cout32 % wn != 0) : (wn != 1 && wn != 2 && wn != 4)) return false;   // packed cout_pad must be a multiple of 32*wn
    if (wm == 2 && (wn > 4 || stride == 2)) return false;
    if (taps == 1 && sc != 32) return false;
    if (stride == 2 && sc != 16) return false;
    return true;
}

// Default choice when the caller gives no tuned variant: minimise modelled time over the menu.
Variant choose_variant(const cmk_conv_desc* descs, int n, int taps, int stride, int cout32) {
    Variant best{1, taps == 1 ? 32 : 16, cout32 <= 7 ? cout32 : 4};
    double best_cost = 1e300;
    const int cout_pad32 = cout32 <= 7 ? cout32 : cdiv(cout32, 4) * 4;
    for (int wn = 7; wn >= 1; --wn)
        for (int wm = 2; wm >= 1; --wm)
            for (int sc = 16; sc <= 32; sc += 16) {
                if (!variant_ok(taps, stride, cout32, wm, sc, wn)) continue;
                const int sr = 32 / sc, bm = 128 * wm;
                const int th = taps == 9 ? sr * 4 * wm : 1, tw = taps == 9 ? sc : bm;
                long blocks = 0;
                for (int i = 0; i < n; ++i) {
                    const int ho = out_size(descs[i].H, stride), wo = out_size(descs[i].W, stride);
                    blocks += taps == 9 ? (long)descs[i].N * cdiv(ho, th) * cdiv(wo, tw) : ((long)descs[i].N * ho * wo + bm - 1) / bm;
                }
                blocks *= cout_pad32 / wn;
                const int apix = taps == 9 ? ((th - 1) * stride + 3) * ((tw - 1) * stride + 3) : bm;
                const int abytes = apix * PST * 4, bbytes = 32 * wn * PST * 4;
                const int occ = occ_of(wm, wn, stride);
                const bool adb = (2 * abytes + 2 * bbytes) * occ <= LDS_CU;
                const int lds = (adb ? 2 : 1) * abytes + 2 * bbytes;
                const int resident = lds * occ <= LDS_CU ? occ : (lds * 2 <= LDS_CU ? 2 : 1);
                // per-workgroup time ~ MFMA cycles per step + a fixed per-step overhead (barrier, LDS fill, address math)
                const double wg_cost = 512.0 * wm * wn + 260.0;
                double cost = round_cost(blocks, resident, wg_cost);
                if (cost < best_cost) { best_cost = cost; best = Variant{wm, sc, wn}; }
            }
    return best;
}

template <int TAPS, int STRIDE, int WN>
static int dispatch_variant(ConvArgs& a, int grid_y, Variant v, hipStream_t st, LaunchPlan* plan) {
    if constexpr (TAPS == 1) {
        if constexpr (WN <= 4) { if (v.wm == 2) return launch<1, 1, 2, WN, 32>(a, grid_y, st, plan); }
        return launch<1, 1, 1, WN, 32>(a, grid_y, st, plan);
    } else if constexpr (STRIDE == 2) {
        return launch<9, 2, 1, WN, 16>(a, grid_y, st, plan);
    } else {
        if constexpr (WN <= 4) {
            if (v.wm == 2) return v.sc == 16 ? launch<9, 1, 2, WN, 16>(a, grid_y, st, plan) : launch<9, 1, 2, WN, 32>(a, grid_y, st, plan);
        }
        return v.sc == 16 ? launch<9, 1, 1, WN, 16>(a, grid_y, st, plan) : launch<9, 1, 1, WN, 32>(a, grid_y, st, plan);
    }
}

template <int TAPS, int STRIDE>
static int dispatch_wn(ConvArgs& a, int cout32, Variant v, hipStream_t st, LaunchPlan* plan) {
    const int cout_pad32 = cout32 <= 7 ? cout32 : cdiv(cout32, 4) * 4;
    a.cout_pad = cout_pad32 * 32;
    const int grid_y = cout_pad32 / v.wn;
    switch (v.wn) {
        case 1: return dispatch_variant<TAPS, STRIDE, 1>(a, grid_y, v, st, plan);
        case 2: return dispatch_variant<TAPS, STRIDE, 2>(a, grid_y, v, st, plan);
        case 3: return dispatch_variant<TAPS, STRIDE, 3>(a, grid_y, v, st, plan);
        case 4: return dispatch_variant<TAPS, STRIDE, 4>(a, grid_y, v, st, plan);
        case 5: return dispatch_variant<TAPS, STRIDE, 5>(a, grid_y, v, st, plan);
        case 6: return dispatch_variant<TAPS, STRIDE, 6>(a, grid_y, v, st, plan);
        case 7: return dispatch_variant<TAPS, STRIDE, 7>(a, grid_y, v, st, plan);
    }
    return fail(CMK_EINVAL, "conv: bad WN%s", "");
}

int launch_igemm(ConvArgs& a, int ksize, int stride, int cout32, Variant v, hipStream_t st, LaunchPlan* plan) {
    if (ksize == 1) return dispatch_wn<1, 1>(a, cout32, v, st, plan);
    if (stride == 1) return dispatch_wn<9, 1>(a, cout32, v, st, plan);
    return dispatch_wn<9, 2>(a, cout32, v, st, plan);
}

int launch_igemm_gather(ConvArgs& a, int wn, int grid_y, hipStream_t st, LaunchPlan* plan) {
    return wn == 4 ? launch<1, 1, 1, 4, 32, true>(a, grid_y, st, plan) : wn == 2 ? launch<1, 1, 1, 2, 32, true>(a, grid_y, st, plan)
                                                                        : launch<1, 1, 1, 1, 32, true>(a, grid_y, st, plan);
}

}  // namespace cmk
