// Winograd F(2x2, 3x3) for 3x3 stride-1 convs (cmk.h tune_wm 5): conv_wino4r_kernel and its launch.  Since the F(4x4) kernels
// (conv_wino6.hip, conv_wino6s.hip) only a fallback: maps their tilings fit badly, Cin % 8 != 0.
#include "conv_args.hpp"

namespace cmk {

// ---------------------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) form for 3x3 stride-1 convs, fused in one kernel (input transform, 16 frequency GEMMs on the
// matrix pipe, output transform all on chip): 2.25x fewer MFMA flops than the direct form, still plain fp32 arithmetic
// (transform matrices hold only 0, +-1, +-1/2; results differ from the direct kernel by fp32 rounding only).
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A        per 4x4 input patch d -> 2x2 outputs, summed over input channels
//   workgroup = 8x16 output pixels (32 tiles of 2x2) x 64 output channels, 4 waves = 2 frequency halves (fh) x 2 cout halves (ng);
//   a wave keeps 8 accumulators of 32 tiles x 32 couts (128 VGPRs), so two workgroups (78 KiB of LDS each) live on a CU and one
//   workgroup's staging / transform / barrier phases hide under the other's MFMAs;
//   per 16-channel chunk: halo (10x18 px) -> LDS, every thread transforms (tile, channel quad) patches into the 16 frequency planes
//   V[f][tile][ci] (16-byte chunks XOR-swizzled, conflict-free ds_read_b128 without padding);
//   a lane of a 32x32 accumulator holds every frequency of its (tile, cout) entries for its half, so the output transform is
//   per-lane register arithmetic; the two frequency halves swap partial sums through LDS once at the end.
// Weights: what bounded the earlier LDS-DMA forms was a latency chain, not throughput — a weight piece could only be requested one
// step ahead (two 16 KiB LDS buffers were all that fit) and an L2 round trip under load is about as long as a step, so every step
// waited for it (a shader-clock trace build of those forms, removed with them; tools/probe/mfma_probe3.hip).  Here each lane loads its own U operand pieces from global memory
// (L2-resident, shared by all workgroups) into registers TWO steps ahead (layout R = one contiguous KiB per wave load,
// cmk_conv_desc.w_wino); the LDS that a weight buffer would take holds a second V buffer, so the input transform of chunk c+1
// overlaps the MFMAs of chunk c with two barriers per chunk, none of which waits for memory.
// ---------------------------------------------------------------------------------------------------------------
constexpr int R_TH = 8, R_TW = 16;                 // outputs of a workgroup's spatial tile
constexpr int R_GN_RECS = 2;                       // fused GroupNorm statistics: one record per (tile, row parity fh, group)
constexpr int S_HALO = 10 * 18;
constexpr int S_SH = S_HALO * PST;                 // floats
constexpr int S_SV = 16 * 32 * 16;
constexpr int S_H_ITERS = (S_HALO * 4 + 255) / 256;
constexpr int R_LDS_BYTES = (S_SH + 2 * S_SV) * 4;
// AFF: the producer's GroupNorm+ReLU is applied while the halo is staged (FCOS tower convs 2-4 and the predictors).  Without it the
// staging registers of the affine are free and the weights are fetched three steps ahead instead of two.
template <bool AFF>
__global__ __launch_bounds__(256, 2) void conv_wino4r_kernel(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sH = smem;
    float* sV = smem + S_SH;                 // two V buffers (chunk parity)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, li = lane & 31;
    const int fh = wave >> 1, ng = wave & 1;

    // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs (each with its own L2), so the grid_y workgroups that
    // share an input tile are given to the SAME XCD, back to back: the tile's halo is fetched into one L2 once.
    // (b % 8 only says which workgroups share an XCD; nothing here depends on it for correctness.)
    const int xq = blockIdx.x >> 3, xcd = blockIdx.x & 7;
    const int bx = (xq / a.grid_y) * 8 + xcd, by = xq % a.grid_y;
    if (bx >= a.total_tiles) return;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAXP; ++i)
        if (i < a.nprob && bx >= a.p[i].tile_begin) pi = i;
    const ConvProblem& P = a.p[pi];
    const int H = P.H, W = P.W;
    const int tile = bx - P.tile_begin;
    const int tw = tile % P.tiles_w;
    const int t2 = tile / P.tiles_w;
    const int th = t2 % P.tiles_h;
    const int n = t2 / P.tiles_h;
    const int oh0 = th * 8, ow0 = tw * 16;
    const int co0 = by * 64;
    const int nchunks = a.Cin >> 4;

    const float* xin = P.x + (long)n * H * W * a.x_cs + a.x_co;
    long g_off[S_H_ITERS];
    unsigned ok = 0;
#pragma unroll
    for (int it = 0; it < S_H_ITERS; ++it) {
        int idx = it * 256 + tid;
        int pix = idx >> 2, q = idx & 3;
        long off = 0;
        if (idx < S_HALO * 4) {
            int hr = pix / 18, hc = pix - hr * 18;
            int ih = oh0 - 1 + hr, iw = ow0 - 1 + hc;
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) { off = ((long)ih * W + iw) * a.x_cs + q * 4; ok |= 1u << it; }
        }
        g_off[it] = off;
    }
    f32x4 h_stage[S_H_ITERS];
    constexpr bool has_aff = AFF;                    // fused GroupNorm apply + ReLU of the producer
    const float* aff_s = has_aff ? P.in_scale + (long)n * a.Cin + (tid & 3) * 4 : nullptr;
    const float* aff_b = has_aff ? P.in_shift + (long)n * a.Cin + (tid & 3) * 4 : nullptr;
    f32x4 in_sc = {1.f, 1.f, 1.f, 1.f}, in_sh = {0.f, 0.f, 0.f, 0.f};
    auto load_H = [&](int chunk) {
#pragma unroll
        for (int it = 0; it < S_H_ITERS; ++it) h_stage[it] = *reinterpret_cast<const f32x4*>(xin + g_off[it] + chunk * 16);
        if (has_aff) {
            in_sc = *reinterpret_cast<const f32x4*>(aff_s + chunk * 16);
            in_sh = *reinterpret_cast<const f32x4*>(aff_b + chunk * 16);
        }
    };
    auto store_H = [&]() {
#pragma unroll
        for (int it = 0; it < S_H_ITERS; ++it) {
            int idx = it * 256 + tid;
            if ((it + 1) * 256 <= S_HALO * 4 || idx < S_HALO * 4) {
                f32x4 v = h_stage[it];
                const bool k = (ok >> it) & 1u;
                if (has_aff) {
                    v.x = fmaxf(v.x * in_sc.x + in_sh.x, 0.f); v.y = fmaxf(v.y * in_sc.y + in_sh.y, 0.f);
                    v.z = fmaxf(v.z * in_sc.z + in_sh.z, 0.f); v.w = fmaxf(v.w * in_sc.w + in_sh.w, 0.f);
                }
                v.x = k ? v.x : 0.f; v.y = k ? v.y : 0.f; v.z = k ? v.z : 0.f; v.w = k ? v.w : 0.f;
                *reinterpret_cast<f32x4*>(sH + (idx >> 2) * PST + (idx & 3) * 4) = v;
            }
        }
    };
    // Weights: same packed U image as the LDS-DMA form ([chunk][ntile][4 steps][4 freq][64 co][16 ci], 16-byte chunks XOR-swizzled),
    // but every lane fetches its own two 16-byte operand pieces per frequency straight into registers (L2-resident, shared by
    // all workgroups): no LDS space, no LDS reads and no DMA drain in front of the barriers.
    const long u_chunk_stride = (long)a.grid_y * 16 * (64 * 16);
    const int t_half = tid >> 7, t_tile = (tid >> 2) & 31, t_q = tid & 3;
    const int t_ty = t_tile >> 3, t_tx = t_tile & 7;
    const int v_chunk = (t_q ^ ((t_tile >> 2) & 3)) * 4;
    // Input transform of one frequency row pair: part 0 -> rows {0, 2} (frequencies 0-3 / 8-11, used by steps 0-1),
    // part 1 -> rows {1, 3} (frequencies 4-7 / 12-15, used by steps 2-3).  Thread half h2 owns rows {2*h2, 2*h2+1}.
    // Row ii of a thread half is p + sg*q of two patch rows (B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]):
    //   half 0: row 0 = d0 - d2, row 1 = d1 + d2;   half 1: row 2 = d2 - d1, row 3 = d1 - d3.
    // The half is wave-uniform, so (p row, q row, sign) are scalars: 8 loads + 16 FMAs per part, no select of two variants.
    const int uhalf = __builtin_amdgcn_readfirstlane(t_half);
    const int prow0 = uhalf ? 2 : 0, qrow0 = uhalf ? 1 : 2;      // part 0 (ii = 0): sign -1 for both halves
    const int prow1 = 1, qrow1 = uhalf ? 3 : 2;                  // part 1 (ii = 1)
    const float sg1 = uhalf ? -1.0f : 1.0f;
    auto transform_part = [&](int ii, int buf) {
        const float* src = sH + ((2 * t_ty) * 18 + 2 * t_tx) * PST + t_q * 4;
        const float* ps = src + (ii == 0 ? prow0 : prow1) * 18 * PST;
        const float* qs = src + (ii == 0 ? qrow0 : qrow1) * 18 * PST;
        const float sg = ii == 0 ? -1.0f : sg1;
        f32x4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 pv = *reinterpret_cast<const f32x4*>(ps + j * PST);
            f32x4 qv = *reinterpret_cast<const f32x4*>(qs + j * PST);
            x[j] = pv + sg * qv;
        }
        f32x4 v0 = x[0] - x[2], v1 = x[1] + x[2], v2 = x[2] - x[1], v3 = x[1] - x[3];
        float* dst = sV + buf * S_SV + (((2 * t_half + ii) * 4) * 32 + t_tile) * 16 + v_chunk;
        *reinterpret_cast<f32x4*>(dst + 0 * 32 * 16) = v0;
        *reinterpret_cast<f32x4*>(dst + 1 * 32 * 16) = v1;
        *reinterpret_cast<f32x4*>(dst + 2 * 32 * 16) = v2;
        *reinterpret_cast<f32x4*>(dst + 3 * 32 * 16) = v3;
    };

    // epilogue scale/shift are fetched here, long before they are needed: loaded in the epilogue (under the cout mask) the compiler's
    // waitcnt bookkeeping could not prove them landed at the joins of the masked store blocks and put `s_waitcnt vmcnt(0)` in front
    // of every one of a lane's 32 global stores, i.e. each store waited for the previous one to retire
    const int co = co0 + ng * 32 + li;
    const bool cvalid = co < a.Cout;
    const float sc = P.scale[min(co, a.Cout - 1)];
    const float sh = P.shift[min(co, a.Cout - 1)];

    f32x16 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[f][r] = 0.f;

    const int sw = (li >> 2) & 3;
    const int c0 = ((2 * hh) ^ sw) * 4, c1 = ((2 * hh + 1) ^ sw) * 4;
    const float* Abase = sV + ((fh * 8) * 32 + li) * 16;
    // register-weight layout R: [chunk][ntile][step 4][fh 2][ng 2][fl 2][piece 2][lane 64][4 floats] — every operand load of a wave is
    // one contiguous KiB (lane = 32*hh + li holds channels 8*hh + 4*piece .. +3 of cout ng*32 + li)
    const float* u_lane = a.w + (long)by * 16 * (64 * 16) + (fh * 2 + ng) * 1024 + lane * 4;
    f32x4 bq[4][2][2];                       // [register buffer: step % 4][fl][operand piece]
    auto load_B = [&](int step, int buf) {   // step = chunk*4 + group: frequencies {2g, 2g+1} of this wave's half
        const float* s = u_lane + (step >> 2) * u_chunk_stride + (step & 3) * (4 * 64 * 16);
#pragma unroll
        for (int fl = 0; fl < 2; ++fl) {
            bq[buf][fl][0] = *reinterpret_cast<const f32x4*>(s + (fl * 2 + 0) * 256);
            bq[buf][fl][1] = *reinterpret_cast<const f32x4*>(s + (fl * 2 + 1) * 256);
        }
    };

    // Schedule: TWO barriers per chunk, 32 MFMAs per wave between them; no barrier waits for a weight load.
    //   steps 0-1 of chunk c: MFMAs on V(c) (buffer c&1) + the input transform of chunk c+1 from the halo into the other V buffer
    //   barrier (everyone is done reading the halo)
    //   steps 2-3: MFMAs + the halo of chunk c+2 registers -> LDS (its global loads were issued in step 0)
    //   barrier (V(c+1) and the new halo are visible; V(c) may be overwritten)
    const int total_steps = nchunks * 4;
    // prologue: the halos of chunks 0 AND 1 and the first weight pieces are requested together, so only one memory round trip is
    // exposed before the first MFMA (chunk 1's halo waits in registers until chunk 0's has been transformed)
    load_H(0);
    f32x4 h_next[S_H_ITERS], sc_next = in_sc, sh_next = in_sh;
    {
        const int c1 = min(1, nchunks - 1);
#pragma unroll
        for (int it = 0; it < S_H_ITERS; ++it) h_next[it] = *reinterpret_cast<const f32x4*>(xin + g_off[it] + c1 * 16);
        if (has_aff) {
            sc_next = *reinterpret_cast<const f32x4*>(aff_s + c1 * 16);
            sh_next = *reinterpret_cast<const f32x4*>(aff_b + c1 * 16);
        }
    }
    // weight operands are fetched PF steps ahead into four register buffers (index = step % 4 = g; a buffer is live for PF steps);
    // the first PF pieces are requested here, with the halos
    constexpr int PF = AFF ? 2 : 3;
#pragma unroll
    for (int t = 0; t < PF; ++t) load_B(min(t, total_steps - 1), t);
    store_H();
    __syncthreads();
    transform_part(0, 0);
    transform_part(1, 0);
#pragma unroll
    for (int it = 0; it < S_H_ITERS; ++it) h_stage[it] = h_next[it];
    in_sc = sc_next; in_sh = sh_next;
    __syncthreads();
    store_H();
    for (int c = 0; c < nchunks; ++c) {
        const int cnn = min(c + 2, nchunks - 1);
        const float* A = Abase + (c & 1) * S_SV;
        const int nbuf = (c + 1) & 1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int step = c * 4 + g;
            const int sb = g, sb2 = (g + PF) & 3;
            if (g == 0 || g == 2) __syncthreads();
            if (g == 0) load_H(cnn);
            load_B(min(step + PF, total_steps - 1), sb2);
            f32x4 a0[2], a1[2];
#pragma unroll
            for (int fl = 0; fl < 2; ++fl) {
                const int al = g * 2 + fl;
                a0[fl] = *reinterpret_cast<const f32x4*>(A + al * 32 * 16 + c0);
                a1[fl] = *reinterpret_cast<const f32x4*>(A + al * 32 * 16 + c1);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int fl = 0; fl < 2; ++fl)
                    acc[g * 2 + fl] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[fl][s], bq[sb][fl][0][s], acc[g * 2 + fl], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int fl = 0; fl < 2; ++fl)
                    acc[g * 2 + fl] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[fl][s], bq[sb][fl][1][s], acc[g * 2 + fl], 0, 0, 0);
            if (g == 0) transform_part(0, nbuf);
            if (g == 1) transform_part(1, nbuf);
            if (g == 2) store_H();
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            if (g == 0 || g == 1) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                }
            } else if (g == 2) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                }
            }
        }
    }

    __syncthreads();
    float2* ex = reinterpret_cast<float2*>(sV);     // [wave 4][r 16][64 lanes] x (dx 0,1) = 32 KiB
    float keep[16][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s0[2], s1[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float m0 = acc[i * 4 + 0][r], m1 = acc[i * 4 + 1][r], m2 = acc[i * 4 + 2][r], m3 = acc[i * 4 + 3][r];
            s0[i] = m0 + m1 + m2;
            s1[i] = m1 - m2 - m3;
        }
        float2 send;
        if (fh == 0) {
            keep[r][0] = s0[0] + s0[1]; keep[r][1] = s1[0] + s1[1];
            send = make_float2(s0[1], s1[1]);
        } else {
            keep[r][0] = -s0[0] - s0[1]; keep[r][1] = -s1[0] - s1[1];
            send = make_float2(s0[0], s1[0]);
        }
        ex[(wave * 16 + r) * 64 + lane] = send;
    }
    __syncthreads();
    const int partner = wave ^ 2;
    const bool do_relu = co < a.relu_upto;
    // accumulator row r of lane half hh is tile (ty, tx) = (r >> 2, (r & 3) + 4*hh): the row offset of a store is uniform per r,
    // only the 8*hh column shift and the channel are per lane -> one lane base pointer, scalar offsets
    const int ow_l = ow0 + 8 * hh;
    float* ybase = P.y + (((long)n * H + oh0 + fh) * W + ow_l) * a.y_cs + a.y_co + co;
    float gs = 0.f, gss = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ty = r >> 2, txr = r & 3;
        const float2 other = ex[(partner * 16 + r) * 64 + lane];
        const bool row_ok = cvalid && (oh0 + 2 * ty + fh < H);
        float* yp = ybase + ((long)(2 * ty) * W + 2 * txr) * a.y_cs;
        float v0 = (keep[r][0] + other.x) * sc + sh, v1 = (keep[r][1] + other.y) * sc + sh;
        if (do_relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
        const bool ok0 = row_ok && ow_l + 2 * txr < W, ok1 = row_ok && ow_l + 2 * txr + 1 < W;
        if (ok0) { yp[0] = v0; gs += v0; gss = fmaf(v0, v0, gss); }
        if (ok1) { yp[a.y_cs] = v1; gs += v1; gss = fmaf(v1, v1, gss); }
    }
    // fused GroupNorm statistics of the NEXT layer's normalisation (fcos.py:182-186): fold the lane's 32 outputs over the
    // channels of its group (adjacent lanes) and the two column halves, one {sum, sumsq} record per (tile, row parity, group)
    if (a.gn_ws) {
        for (int o = 1; o < a.gn_cpg; o <<= 1) { gs += __shfl_xor(gs, o); gss += __shfl_xor(gss, o); }
        gs += __shfl_xor(gs, 32);
        gss += __shfl_xor(gss, 32);
        if (cvalid && hh == 0 && (li & (a.gn_cpg - 1)) == 0) {
            double* o = a.gn_ws + (((long)bx * R_GN_RECS + fh) * a.gn_groups + co / a.gn_cpg) * 2;
            o[0] = (double)gs;
            o[1] = (double)gss;
        }
    }
}

int wino4r_gn_records(int H, int W) { return R_GN_RECS * cdiv(H, R_TH) * cdiv(W, R_TW); }

int launch_wino4r(ConvArgs& a, hipStream_t st, LaunchPlan* plan) {
    static DeviceOnce once;
    int rc0 = plan ? CMK_OK : once.run([]() {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wino4r_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, R_LDS_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wino4r_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, R_LDS_BYTES);
        return e == hipSuccess ? CMK_OK : fail(CMK_ELAUNCH, "conv_wino: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    });
    if (rc0) return rc0;
    int blocks = 0;
    for (int i = 0; i < a.nprob; ++i) {
        ConvProblem& p = a.p[i];
        p.tile_begin = blocks;
        p.tiles_h = cdiv(p.Ho, R_TH);
        p.tiles_w = cdiv(p.Wo, R_TW);
        blocks += p.N * p.tiles_h * p.tiles_w;
    }
    a.grid_y = cdiv(a.Cout, 64);
    a.total_tiles = blocks;
    if (plan) {      // a workgroup: 16 frequency GEMMs of 32 tiles (2x2 outputs each) x 64 couts over Cin
        snprintf(plan->kernel, sizeof(plan->kernel), "conv_wino4r_kernel<%s>", tf(a.p[0].in_scale));
        plan->executed_flops = 2 * (int64_t)blocks * a.grid_y * 16 * (R_TH * R_TW / 4) * 64 * a.Cin;
        for (int i = 0; i < a.nprob; ++i) plan->gn_records[i] = a.gn_ws ? wino4r_gn_records(a.p[i].Ho, a.p[i].Wo) : 0;
        return CMK_OK;
    }
    const dim3 grid(((blocks + 7) / 8) * 8 * a.grid_y);
    if (a.p[0].in_scale)          // all problems of a launch agree on this (validated)
        hipLaunchKernelGGL(conv_wino4r_kernel<true>, grid, dim3(256), R_LDS_BYTES, st, a);
    else
        hipLaunchKernelGGL(conv_wino4r_kernel<false>, grid, dim3(256), R_LDS_BYTES, st, a);
    return check_launch("conv_wino");
}

}  // namespace cmk
