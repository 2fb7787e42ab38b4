// Shared by the Winograd F(4x4,3x3) kernels (conv_wino6.hip: 32 couts per workgroup, two workgroups per CU, and its paired form, 64 couts
// per workgroup from one shared W image; conv_wino6s.hip: 64 couts per workgroup with the frequency image V shared through LDS): tile geometries, the conflict-free W-image slot function and the
// packed-fp32 half transforms, the output transform (w6_epilogue: the one epilogue of all three kernels) and the host side's tile walk and
// geometry refusals.
#pragma once
#include <type_traits>

#include "conv_args.hpp"

namespace cmk {

// Two tilings of the 32 MFMA rows (a workgroup's 32 tiles of 4x4 outputs):
//   GEO 0  maps: 3 x 10 tiles of ONE image (12 x 40 pixels: every map width of the model is a multiple of 40); rows 30, 31 carry no tile;
//   GEO 1  RoI maps (at most 16 rows x 14 columns, e.g. the 14x14 RoI features of the mask / mask-IoU heads): 4 x 4 tiles of each of
//          TWO consecutive images; halo columns 15..17 (image columns >= 14) are zero by construction, so their W slots are cleared
//          once and only 15 columns go through pass 1: 2 x (4 x 15 x 2) = 240 items, waves 0-1 image 0, waves 2-3 image 1.
// W image, in 16-byte slots: entry (channel quad q, row group r, grid row a, halo column col) lives at
//   q*QP + r*TP + a*AP + (col & 3)*CK + (col >> 2)          r = tile row (GEO 0) or 4*image + tile row (GEO 1)
// A lane of the MFMA side is tile m and reads col = 4*tc + j, i.e. slot = const + r*TP + tc (+1 for j >= 4).  A ds_read_b128 is served
// in groups of 16 lanes {0-3,12-15,20-27} / {4-11,16-19,28-31} per half wave; TP is chosen modulo 16 (10 for GEO 0, 4 for GEO 1) so that
// the tiles of either group fall on 16 distinct slots modulo 16, whatever a and j are: conflict-free without padding the rows.
template <int GEO> struct W6G;
template <> struct W6G<0> {
    static constexpr int OH = 12, OW = 40, HC = 42, CK = 12, AP = 48, TP = 6 * 48 + 10, RG = 3, QP = RG * TP, WB = 2 * QP;
    static constexpr int ITEMS = 3 * HC * 2;                // 252: (tile row, halo column, channel quad)
    static constexpr int TILES = 30;
    __device__ static __forceinline__ void tile_of(int m, int& img, int& t, int& tc) { img = 0; t = (m * 205) >> 11; tc = m - t * 10; }      // m / 10, m < 32
    __device__ static __forceinline__ void item_of(int tid, int& img, int& q, int& t, int& col, bool& active) {
        const int i = min(tid, ITEMS - 1);                 // threads 252..255 repeat the last item (same values, same slots)
        img = 0; q = i & 1; const int cc = i >> 1; t = cc / HC; col = cc - t * HC; active = true;
    }
};
template <> struct W6G<1> {
    static constexpr int OH = 16, OW = 14, HC = 15, CK = 5, AP = 20, TP = 6 * 20 + 12, RG = 8, QP = RG * TP, WB = 2 * QP;
    static constexpr int ITEMS = 256;
    static constexpr int TILES = 32;
    __device__ static __forceinline__ void tile_of(int m, int& img, int& t, int& tc) { img = m >> 4; t = (m >> 2) & 3; tc = m & 3; }
    __device__ static __forceinline__ void item_of(int tid, int& img, int& q, int& t, int& col, bool& active) {
        img = tid >> 7; const int i = tid & 127; active = i < 4 * HC * 2;
        const int j = min(i, 4 * HC * 2 - 1); q = j & 1; const int cc = j >> 1; t = cc / HC; col = cc - t * HC;
    }
};
static_assert(W6G<0>::TP % 16 == 10 && W6G<1>::TP % 16 == 4, "conflict-free W image");
constexpr int W6_GN_RECS = 4;      // fused GroupNorm statistics: one record per (spatial tile, wave g of the cout tile, group)
// a wave-group's work on one spatial tile, one 32-cout tile and one channel: 36 frequency GEMMs of 32 tiles (4x4 outputs each) x 32 couts
constexpr int64_t W6_FLOPS_PER_CHANNEL = 2 * 36 * 32 * 32;

template <int GEO>
__device__ __forceinline__ int w6_slot(int q, int r, int a, int col) {
    using G = W6G<GEO>;
    return q * G::QP + r * G::TP + a * G::AP + (col & 3) * G::CK + (col >> 2);
}

// Tail split-K (conv_args.hpp): the 8-channel chunks [c_lo, c_hi) of piece `piece` of `ways`.  The chunk loop runs two periods per trip, so
// a piece gets whole chunk PAIRS, spread as evenly as the count allows (floor bounds: sizes differ by at most one pair; 17 pairs of the
// 272-channel MaskIoU conv in 8 ways = 2,2,2,2,2,2,2,3).  Where chunks % (2 * ways) == 0 these are the bounds of ordinary split-K.
__host__ __device__ __forceinline__ void w6_piece_bounds(int chunks, int ways, int piece, int& c_lo, int& c_hi) {
    const unsigned pairs = (unsigned)chunks >> 1;
    c_lo = (int)(2u * ((unsigned)piece * pairs / (unsigned)ways));
    c_hi = piece + 1 == ways ? chunks : (int)(2u * ((unsigned)(piece + 1) * pairs / (unsigned)ways));
}

// Packed-fp32 arithmetic spelled out.  The transforms are the minimal sequences of v_pk_* instructions (6 per half transform of two
// channels); left to the compiler the same formulas came out as a mix of scalar FMAs, sign flips (v_xor) and register moves — 5.5 VALU
// instructions per MFMA instead of 1.5.  One asm block per half transform: the compiler cannot see what kind of instruction wrote the
// results, so it cannot keep its own distance rules between a VALU write and the MFMA / LDS store that reads it (built from single-
// instruction asm statements the kernel computed garbage as soon as the scheduler moved them); the block ends with the wait states itself.
//   first  (B^T rows 0-2 on x0..x4 = d0..d4):  v0 = 4x0 - 5x2 + x4,  v1 = (x4 - 4x2) + (x3 - 4x1),  v2 = (x4 - 4x2) - (x3 - 4x1)
//   second (B^T rows 3-5 on x0..x4 = d1..d5):  v0 = (x3 - x1) + 2(x2 - x0),  v1 = (x3 - x1) - 2(x2 - x0),  v2 = 4x0 - 5x2 + x4
__device__ __forceinline__ void w6_half_first(const f32x2 x0, const f32x2 x1, const f32x2 x2, const f32x2 x3, const f32x2 x4, const f32x2 five,
                                              f32x2& v0, f32x2& v1, f32x2& v2) {
    f32x2 p, q;
    asm volatile("v_pk_fma_f32 %0, %7, %10, %9 op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"      // v0 = x4 - 5 x2
                 "v_pk_fma_f32 %3, %7, 4.0, %9 op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"       // p  = x4 - 4 x2
                 "v_pk_fma_f32 %4, %6, 4.0, %8 op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"       // q  = x3 - 4 x1
                 "v_pk_fma_f32 %0, %5, 4.0, %0 op_sel_hi:[1,0,1]\n\t"                                      // v0 += 4 x0
                 "v_pk_add_f32 %1, %3, %4\n\t"                                                             // v1 = p + q
                 "v_pk_add_f32 %2, %3, %4 neg_lo:[0,1] neg_hi:[0,1]\n\t"                                   // v2 = p - q
                 "s_nop 1"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(p), "=&v"(q)
                 : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(x4), "s"(five));
}
__device__ __forceinline__ void w6_half_second(const f32x2 x0, const f32x2 x1, const f32x2 x2, const f32x2 x3, const f32x2 x4, const f32x2 five,
                                               f32x2& v0, f32x2& v1, f32x2& v2) {
    f32x2 r, t;
    asm volatile("v_pk_add_f32 %3, %8, %6 neg_lo:[0,1] neg_hi:[0,1]\n\t"                                   // r  = x3 - x1
                 "v_pk_add_f32 %4, %7, %5 neg_lo:[0,1] neg_hi:[0,1]\n\t"                                   // t  = x2 - x0
                 "v_pk_fma_f32 %2, %7, %10, %9 op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"      // v2 = x4 - 5 x2
                 "v_pk_fma_f32 %0, %4, 2.0, %3 op_sel_hi:[1,0,1]\n\t"                                      // v0 = r + 2t
                 "v_pk_fma_f32 %1, %4, 2.0, %3 op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"       // v1 = r - 2t
                 "v_pk_fma_f32 %2, %5, 4.0, %2 op_sel_hi:[1,0,1]\n\t"                                      // v2 += 4 x0
                 "s_nop 1"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(r), "=&v"(t)
                 : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(x4), "s"(five));
}

// Where w6_epilogue stores: finished values into the conv's output view (raw = std::false_type or false), or raw partial sums into a split-K /
// tail slab of the workspace, laid out [pixel][cout_pad], for the reduce kernel (conv.hip) to sum in a fixed order and finish.  The struct
// only NAMES the target; the epilogue turns it into a buffer, strides and an image index where it needs them, behind its barrier (worked
// out by the caller, the scalar loads and multiplies of the slab address ran in front of the scale/shift loads and the barrier).
template <class RAW> struct W6Out {
    RAW raw;        // this workgroup leaves raw partial sums (no scale / shift / ReLU) in its slab of a.ws
    int piece;      // raw: which of the split's slabs
    int n0;         // raw: the slab's first image (a tail's slabs hold the tail's images alone)
};

// ---- epilogue of conv_wino6_kernel, conv_wino6p_kernel and conv_wino6s_kernel --------------------------------------------------------
// A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1].  Row pass in registers: per accumulator entry the wave's 6 + 3
// frequencies become P[rowA][0..3] and the partial P[rowB][0..3] of its half (the two halves add up).  The four waves g = 0..3 of a cout
// tile swap those through their 64 KiB exchange area ([src wave][dst wave][value 0..7][lane] pairs) in two rounds; wave d finishes the
// tiles of accumulator registers 4d..4d+3: in round q the other waves send it the 8 values of registers 4d+2q, 4d+2q+1.  Then column pass,
// scale/shift/ReLU, NHWC stores and the GroupNorm statistics.
// act: this wave has a cout tile (wave-uniform; std::true_type where every wave has one).  Waves without one skip the arithmetic and the
// stores but reach every barrier.  (n, oh0, ow0): origin of the workgroup's spatial tile bx in its H x W image; co0: the wave's first
// output channel.  The exchange area is given as the LDS base and an offset in floats, and the pointer is formed here, next to its
// indices: formed by the caller the compiler no longer folds the constant part of an index into the ds instruction's offset field
// (+40 address instructions per kernel).
// Everything works on PAIRS of accumulator registers (r, r+1 = two tiles of the lane) with packed-fp32 instructions, and the stores of
// interior tiles take a wave-uniform (row, column) base from the scalar unit plus one lane offset per tile: a VALU instruction issued here
// waits for a gap in the MFMA stream of the other workgroup on the SIMD and takes the slot from it (trace: this epilogue ran 12.4 us next
// to a partner, 5.6 us alone), so the epilogue is priced in VALU instructions — 3x fewer than the scalar form.
template <int GEO, class ACT, class RAW>
__device__ __forceinline__ void w6_epilogue(const ConvArgs& a, const ConvProblem& P, f32x16 (&acc)[9], float* const smem, const int ex_floats, const int g, const int lane,
                                            const int li, const int hh, const ACT act, const int co0, const int H, const int W, const int n, const int oh0, const int ow0,
                                            const int bx, const W6Out<RAW> out) {
    using G = W6G<GEO>;
    const int halfB = g & 1;
    // scale/shift are requested here: the two exchange rounds cover their latency (loaded inside the store loop they would serialise it)
    const int co = co0 + li;
    const bool cvalid = act && co < a.Cout;
    float sc = P.scale[min(co, a.Cout - 1)];
    float sh = P.shift[min(co, a.Cout - 1)];
    __syncthreads();
    // The stores below sit in per-tile predicated blocks; the compiler's wait-count pass cannot prove across their joins that the two loads
    // above have landed and would put `s_waitcnt vmcnt(0)` in front of every store — which also waits for the previous STORE to retire
    // (measured: 340 ns per store, 26 us of a 76 us workgroup).  Wait once here and hand the values over through an asm the pass
    // cannot see through: from now on they are plain register values.
    asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, %0\n\tv_mov_b32 %1, %1" : "+v"(sc), "+v"(sh) : : "memory");
    f32x2* ex2 = reinterpret_cast<f32x2*>(smem + ex_floats);
    // raw is a property of the WORKGROUP: with a tail (GEO 1) only its pieces are raw; their slabs hold the tail's images alone, so a piece
    // stores image n at slab image n - n0, and the main part's workgroups store finished values to y as ever
    const bool raw = out.raw;
    const long slab_pix = GEO == 1 ? (long)(P.N - out.n0) * H * W : P.total_pix;
    float* const ybuf = raw ? a.ws + (long)out.piece * slab_pix * a.cout_pad : P.y;
    const int n_st = n - out.n0;
    const int ycs = raw ? a.cout_pad : a.y_cs, yco = raw ? 0 : a.y_co;
    if (raw) { sc = 1.f; sh = 0.f; }
    const float lo = (co < a.relu_upto && !raw) ? 0.f : __builtin_nanf("");      // max(v, NaN) = v: lanes without the ReLU
    const f32x2 sc2 = {sc, sc}, sh2 = {sh, sh};
    auto fma2 = [](f32x2 x, float k, f32x2 y) { return __builtin_elementwise_fma(x, f32x2{k, k}, y); };
    const bool want_stats = a.gn_ws != nullptr;
    f32x2 gs2 = {0.f, 0.f}, gss2 = {0.f, 0.f};
    float gs = 0.f, gss = 0.f;
    float* yimg = ybuf + (long)n_st * H * W * ycs + yco + co;
    // scalar side of the store addresses: image base (the pair's first image for GEO 1) and the byte strides of one pixel / one row
    const unsigned long long ybase_s = wave_uniform_u64(ybuf + (long)n_st * H * W * ycs);
    const unsigned long long px_b = (unsigned long long)ycs * 4u, rowskip_b = (unsigned long long)(W - 3) * ycs * 4u;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        f32x2 own[8];
        if (act) {
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const int r0 = 4 * dd + 2 * q;
                f32x2 v[8];
                {
                    const f32x2 m0 = {acc[0][r0], acc[0][r0 + 1]}, m1 = {acc[1][r0], acc[1][r0 + 1]}, m2 = {acc[2][r0], acc[2][r0 + 1]},
                                m3 = {acc[3][r0], acc[3][r0 + 1]}, m4 = {acc[4][r0], acc[4][r0 + 1]}, m5 = {acc[5][r0], acc[5][r0 + 1]};
                    const f32x2 s1 = m1 + m2, d1 = m1 - m2, s2 = m3 + m4, d2 = m3 - m4;
                    v[0] = m0 + s1 + s2;
                    v[1] = fma2(d2, 2.0f, d1);
                    v[2] = fma2(s2, 4.0f, s1);
                    v[3] = fma2(d2, 8.0f, d1) + m5;
                    const f32x2 n0 = {acc[6][r0], acc[6][r0 + 1]}, n1 = {acc[7][r0], acc[7][r0 + 1]}, n2 = {acc[8][r0], acc[8][r0 + 1]};
                    if (halfB == 0) {      // b = 0, 1, 2
                        const f32x2 t1 = n1 + n2, e1 = n1 - n2;
                        v[4] = n0 + t1; v[5] = e1; v[6] = t1; v[7] = e1;
                    } else {               // b = 3, 4, 5
                        const f32x2 t2s = n0 + n1, e2 = n0 - n1;
                        v[4] = t2s; v[5] = e2 + e2; v[6] = t2s * 4.0f; v[7] = fma2(e2, 8.0f, n2);
                    }
                }
                if (dd == g) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) own[k] = v[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) ex2[(((g * 4 + dd) * 8 + k) << 6) + lane] = v[k];
                }
            }
        }
        __syncthreads();
        if (act) {
            // P[a][j]: rows 0..3 from waves 0..3 (values 0..3), row 4 = halves of waves 0, 1, row 5 = halves of waves 2, 3 (values 4..7)
            f32x2 Pm[6][4];
            {
                f32x2 part[4][4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    f32x2 v[8];
                    if (s == g) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] = own[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] = ex2[(((s * 4 + g) * 8 + k) << 6) + lane];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) { Pm[s][j] = v[j]; part[s][j] = v[4 + j]; }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) { Pm[4][j] = part[0][j] + part[1][j]; Pm[5][j] = part[2][j] + part[3][j]; }
            }
            f32x2 yv[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 s1 = Pm[1][j] + Pm[2][j], d1 = Pm[1][j] - Pm[2][j], s2 = Pm[3][j] + Pm[4][j], d2 = Pm[3][j] - Pm[4][j];
                f32x2 y[4];
                y[0] = Pm[0][j] + s1 + s2;
                y[1] = fma2(d2, 2.0f, d1);
                y[2] = fma2(s2, 4.0f, s1);
                y[3] = fma2(d2, 8.0f, d1) + Pm[5][j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f32x2 t = __builtin_elementwise_fma(y[i], sc2, sh2);
                    t.x = fmaxf(t.x, lo);
                    t.y = fmaxf(t.y, lo);
                    yv[i][j] = t;
                }
            }
            // the pair's entries are accumulator registers 4*g + 2q, +1 of lane half hh: tiles m, m + 1
            bool full[2];
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int m = 2 * q + rr + 8 * g + 4 * hh;
                int mimg, mt, mtc;
                G::tile_of(m, mimg, mt, mtc);
                const int oh = oh0 + 4 * mt, ow = ow0 + 4 * mtc;
                const bool tile_ok = cvalid && m < G::TILES && n + mimg < P.N;
                full[rr] = tile_ok && oh + 4 <= H && ow + 4 <= W;
                if (full[rr]) {                             // interior tile: 16 stores, no per-store predicate, no vector address arithmetic
                    const unsigned voff = (unsigned)((((mimg * H + oh) * W + ow) * ycs + yco + co) * 4);
                    unsigned long long sp = ybase_s;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float val = rr ? yv[i][j].y : yv[i][j].x;
                            // ("+s": the pointer is walked between the stores, not computed 16 times up front)
                            // nt: the output is a stream (84 MB per launch at stage 2) that must not push the weights and the halo lines this launch
                            // re-reads out of L2; measured -2.2 % on the map shapes, +0.4 % end to end (profiles/r03_ablations.txt), sc0 / sc1 nothing
                            asm volatile("global_store_dword %1, %2, %0 nt" : "+s"(sp) : "v"(voff), "v"(val) : "memory");
                            sp += j == 3 ? rowskip_b : px_b;
                        }
                } else if (tile_ok) {
                    float* yp0 = yimg + (((long)mimg * H + oh) * W + ow) * ycs;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (oh + i < H && ow + j < W) {
                                const float val = rr ? yv[i][j].y : yv[i][j].x;
                                yp0[((long)i * W + j) * ycs] = val;
                                gs += val;
                                gss = fmaf(val, val, gss);
                            }
                }
            }
            if (want_stats) {                               // whole tiles: packed, masked by tile
                const f32x2 mask = {full[0] ? 1.f : 0.f, full[1] ? 1.f : 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x2 t = yv[i][j] * mask;
                        gs2 += t;
                        gss2 = __builtin_elementwise_fma(t, yv[i][j], gss2);
                    }
            }
        }
        if (q == 0) __syncthreads();                        // the exchange buffer is reused by round 1
    }
    gs += gs2.x + gs2.y;
    gss += gss2.x + gss2.y;
    // fused GroupNorm statistics of the NEXT layer's normalisation (fcos.py:182-186): one {sum, sumsq} record per
    // (spatial tile, wave g of the cout tile, group of channels)
    if (a.gn_ws && act) {
        for (int o = 1; o < a.gn_cpg; o <<= 1) { gs += __shfl_xor(gs, o); gss += __shfl_xor(gss, o); }
        gs += __shfl_xor(gs, 32);
        gss += __shfl_xor(gss, 32);
        if (cvalid && hh == 0 && (li & (a.gn_cpg - 1)) == 0) {
            double* o = a.gn_ws + (((long)bx * W6_GN_RECS + g) * a.gn_groups + co / a.gn_cpg) * 2;
            o[0] = (double)gs;
            o[1] = (double)gss;
        }
    }
}

// ---- host side, shared by launch_wino6 and launch_wino6s --------------------------------------------------------------------------------
// The spatial tiles of a launch: GEO 0 12x40-pixel tiles of every image, GEO 1 pairs of whole images.  Sets each problem's tile counts and
// tile_begin and returns the total.
template <int GEO>
inline int w6_assign_tiles(ConvArgs& a) {
    int blocks = 0;
    for (int i = 0; i < a.nprob; ++i) {
        ConvProblem& p = a.p[i];
        p.tile_begin = blocks;
        if (GEO == 0) {
            p.tiles_h = cdiv(p.Ho, W6G<0>::OH);
            p.tiles_w = cdiv(p.Wo, W6G<0>::OW);
            blocks += p.N * p.tiles_h * p.tiles_w;
        } else {
            p.tiles_h = p.tiles_w = 1;
            blocks += cdiv(p.N, 2);
        }
    }
    return blocks;
}

// What the leaf launchers of the three kernels leave in a plan (conv_args.hpp) for `blocks` spatial tiles x `cout_tiles` executed 32-cout
// tiles; records: the map geometry's, where the launch writes statistics (the RoI-pair geometry refuses them).
template <int GEO>
inline int w6_plan(LaunchPlan* plan, const ConvArgs& a, const char* kernel, int blocks, int cout_tiles) {
    snprintf(plan->kernel, sizeof(plan->kernel), "%s<%s, %d>", kernel, tf(a.p[0].in_scale), GEO);
    plan->executed_flops = (int64_t)blocks * cout_tiles * a.Cin * W6_FLOPS_PER_CHANNEL;
    for (int i = 0; i < a.nprob; ++i) plan->gn_records[i] = a.gn_ws && GEO == 0 ? W6_GN_RECS * a.p[i].tiles_h * a.p[i].tiles_w : 0;
    return CMK_OK;
}

// What kernel `name` refuses.  The epilogue's stores take a 32-bit byte offset inside the output image (geo 1: inside a pair of images)
// of pixel stride cs.
inline int w6_refuse_size(const ConvArgs& a, int geo, int cs, const char* name) {
    for (int i = 0; i < a.nprob; ++i)
        if ((long)(geo == 0 ? 1 : 2) * a.p[i].H * a.p[i].W * cs * 4 >= (1L << 32))
            return fail(CMK_EINVAL, "%s: an output image of 4 GiB or more", name);
    return CMK_OK;
}
// The RoI-pair geometry: pairs of whole maps of at most 16 rows x 14 columns, one problem, no fused GN statistics.  subject: the head
// of the sentence, "<kernel>: the RoI-pair geometry ..."
inline int w6_refuse_roi_pairs(const ConvArgs& a, const char* subject) {
    if (a.nprob != 1 || a.p[0].H > 16 || a.p[0].W > 14 || a.gn_ws)
        return fail(CMK_EINVAL, "%s takes one problem of maps up to 16x14 and produces no GroupNorm statistics", subject);
    return CMK_OK;
}

}  // namespace cmk
