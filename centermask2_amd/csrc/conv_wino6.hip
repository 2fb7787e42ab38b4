// Winograd F(4x4, 3x3) for 3x3 stride-1 convs, fused in one kernel, plain fp32 on the CDNA4 matrix pipe.
//
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A    per 6x6 input patch d -> 4x4 outputs, summed over input channels: 36 multiplies per
//   16 outputs = 2.25 per output against 9 (direct) and 4 (F(2x2,3x3), conv_wino4r_kernel) — 1.78x fewer MFMAs than the 2x2 form.
//   Interpolation points 0, +-1, +-2, inf (Lavin & Gray); every transform is exact-coefficient fp32 arithmetic, U = G g G^T is
//   computed on the host in fp64 and rounded once.  Measured error of this form on the full model (tools/wino_numerics.py, CPU
//   emulation of exactly this arithmetic): features/logits rms 1.6e-6 relative (F(2x2): 1.0e-6), labels and locations identical.
//
// Shape of the kernel (what differs from conv_wino4r_kernel, and why):
//   * workgroup = 3 x 10 tiles of 4x4 outputs (12 x 40 pixels: every map width of the model is a multiple of 40) x 32 output
//     channels, 4 waves, two workgroups per CU.  30 of the 32 MFMA rows carry a tile.  The 36 frequencies of the 6x6 grid are 36
//     accumulators of 32 tiles x 32 couts; a wave owns 9: grid row a = wave (6 frequencies) and half of row 4 or 5 (3 frequencies).
//     144 accumulator VGPRs per lane — the register budget shapes everything else.
//   * the input transform is split.  B^T d B = (column pass) then (row pass):
//       pass 1 (once per workgroup and 8-channel chunk): thread = (tile row t, halo column, channel quad) — 3 x 42 x 2 = 252 items —
//         loads the 6 input rows of its item straight from global memory into registers one period ahead (buffer loads: rows and
//         columns outside the image come back as 0 from the hardware range check, no masks), forms W[t][a][col] = sum_i B^T[a][i] d[4t+i][col]
//         in place and writes the W image to LDS (28 KiB per chunk, two buffers).  The column pass is shared by horizontally adjacent
//         tiles, and there is no raw-halo stage in LDS at all;
//       pass 2 (by the MFMA waves, in registers, right in front of the MFMAs): a lane reads the 5 W values of its tile that one half of
//         a frequency row needs (conflict-free image, see w6_slot) and forms 3 frequencies with 6 FMAs per channel.
//     So the 36-plane V image (74 KiB per 16 channels — it would not fit twice beside a second workgroup) never exists, LDS traffic per
//     MFMA is a fraction of the 2x2 kernel's, and ONE barrier per chunk (36 MFMAs per wave) is enough — it never waits for memory.
//   * VALU instructions are the currency: fp32 MFMA and VALU do not co-execute here and a period costs 2 waves x (36 MFMAs x 64 +
//     N_valu x ~8) cycles.  A wave issues 60 packed transform instructions + 4 others per period (hand-written v_pk_* blocks, row-B sample
//     addresses set up once, two periods per trip so that the W buffer is a compile-time offset); the fused-affine variant adds 48.
//   * weights never touch LDS: U is packed so that every operand load of a wave is one contiguous KiB ([chunk][cout tile][wave][9][lane][4])
//     and is fetched two steps (24 MFMAs) ahead into registers, as in the 2x2 kernel.
//   * epilogue (w6_epilogue in wino6_common.hpp, shared with conv_wino6s.hip): each wave reduces its frequencies along b in registers (6 -> 4 and 3 -> 4 partial values per entry), the four waves swap
//     those through LDS in two rounds, and wave w finishes the 8 tiles of accumulator registers 4w..4w+3: column pass, scale/shift/ReLU,
//     NHWC stores, GroupNorm statistics — on pairs of accumulator registers with packed fp32, interior tiles stored through a scalar-walked
//     base + one lane offset per tile (~460 VALU instructions per wave; the scalar form took ~1080 and 12.4 us beside a partner's MFMAs).
//
// Paired form (conv_wino6p_kernel, cmk.h tune_sc 32): ONE workgroup of 8 waves per CU covers a spatial tile x 64 couts — waves 0-3 are
// cout tile 2j, waves 4-7 cout tile 2j+1, each wave exactly a conv_wino6 wave (9 frequencies x 32 tiles x 32 couts, pass 2 in its own
// registers, the same weights, the same barrier per chunk).  Only what every cout tile of a spatial tile used to repeat is shared: the
// halo loads, pass 1 and the fused input affine run once per 64 couts, spread over all 512 threads — thread = (pass-1 item, channel
// pair), so each holds half a conv_wino6 thread's halo registers and does half its pass-1 work.  The W image is the same (two buffers),
// the two halves use disjoint epilogue exchange areas.  Same values in the same order: bit-identical to conv_wino6_kernel.
//
// Reference call sites replaced: the same 3x3 stride-1 convs as the 2x2 kernel (vovnet.py:205-219, d2 FPN outputs, fcos.py:169-200,
// sam.py:58-70, maskiou_head.py:81-88).
#include <type_traits>

#include "wino6_common.hpp"

namespace cmk {

constexpr int W6_EX_FLOATS = 4 * 4 * 2 * 8 * 64;       // epilogue exchange: [src wave][dst wave][value][lane][register pair of the round] = 64 KiB
// PAIR: one exchange area per cout tile
template <int GEO, bool PAIR = false> constexpr int w6_lds_bytes() {
    return (2 * W6G<GEO>::WB * 16 > (PAIR ? 2 : 1) * W6_EX_FLOATS * 4) ? 2 * W6G<GEO>::WB * 16 : (PAIR ? 2 : 1) * W6_EX_FLOATS * 4;
}
static_assert(2 * w6_lds_bytes<0>() <= LDS_CU && 2 * w6_lds_bytes<1>() <= LDS_CU, "two workgroups per CU");
static_assert(w6_lds_bytes<0, true>() <= LDS_CU && w6_lds_bytes<1, true>() <= LDS_CU, "paired form: one workgroup per CU");

// AFF: the producer's GroupNorm+ReLU is applied to the input in pass 1 (FCOS tower convs 2-4 and the predictors)
// PAIR: the paired form (header); false = conv_wino6_kernel
template <bool AFF, int GEO, bool PAIR>
__device__ __forceinline__ void conv_wino6_body(const ConvArgs& a) {
    using G = W6G<GEO>;
    constexpr int W6_AP = G::AP, W6_WB = G::WB;
    constexpr int NT = PAIR ? 512 : 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4* sW = reinterpret_cast<f32x4*>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave = PAIR ? (wid & 3) : wid;                     // the wave's place in its cout tile: what conv_wino6 calls the wave
    const int half = PAIR ? (wid >> 2) : 0;                      // PAIR: which of the workgroup's two cout tiles
    const int hh = lane >> 5, li = lane & 31;

    // XCD-aware order, as in the other conv kernels: the grid_y cout tiles of one spatial tile go to the same XCD, back to back
    // (PAIR: the ceil(grid_y / 2) pairs of them)
    const int gy = PAIR ? (a.grid_y + 1) >> 1 : a.grid_y;
    const int xq = blockIdx.x >> 3, xcd = blockIdx.x & 7;
    // (the opposite, weight-stationary mapping — XCD k takes the cout tiles == k mod 8 of every spatial tile so that its L2 holds 1/8 of
    // U — was measured 3-4 % slower on the 256 -> 256 layers: every XCD then reads the whole input)
    int bx = (xq / gy) * 8 + xcd, by = xq % gy;
    // split-K: this workgroup is piece ks of nsplit of its (spatial tile, cout tile): it owns a range of the conv's Cin / 8 chunks and leaves
    // raw partial sums in a.ws (see the epilogue).  Two forms.  Whole launches (GEO 0, a.ksplit > 1, blockIdx.y): launches of about one round
    // of workgroups whose life is one long chunk loop (the first conv of a stage-4 / stage-5 OSA block: 512..1024 input channels on 50x80 /
    // 25x40 maps).  The TAIL of a launch (GEO 1, a.tail_ksplit > 1): the blocks from a.main_blocks on are the pieces of the last
    // a.tail_tiles spatial tiles — (tile, cout tile, piece) decoded like the main part with the piece between them, so the pieces of a
    // tile share its XCD — and being the last blocks of the grid they fill the ragged last round of the chip with short workgroups.
    int ks = blockIdx.y, nsplit = a.ksplit;
    int tile_end = a.total_tiles;       // GEO 1: the main part's tiles end where the tail's begin
    int n_ws = 0;                       // GEO 1, tail: the first image of the tail (slab image indices are relative to it)
    if constexpr (GEO == 1) {
        ks = 0; nsplit = 1;
        const int main_tiles = a.total_tiles - a.tail_tiles;
        tile_end = main_tiles;
        if ((int)blockIdx.x >= a.main_blocks) {
            const int tb = (int)blockIdx.x - a.main_blocks;
            const int tq = tb >> 3, q2 = tq / gy;
            by = tq % gy;
            nsplit = a.tail_ksplit;
            ks = q2 % nsplit;
            bx = main_tiles + (q2 / nsplit) * 8 + (tb & 7);
            tile_end = a.total_tiles;
            n_ws = 2 * main_tiles;
        }
    }
    // this wave's 32-cout tile.  PAIR with an odd number of tiles: the upper half of the last pair has none; it reads the weights of the
    // last tile (ct), computes, and stores nothing (co0 >= Cout)
    const int ctile = PAIR ? 2 * by + half : by;
    const int ct = PAIR ? min(ctile, a.grid_y - 1) : by;
    if (bx >= tile_end) return;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAXP; ++i)
        if (i < a.nprob && bx >= a.p[i].tile_begin) pi = i;
    const ConvProblem& P = a.p[pi];
    const int H = P.H, W = P.W;
    const int tile = bx - P.tile_begin;
    int n, oh0, ow0;
    if (GEO == 0) {
        const int tw = tile % P.tiles_w;
        const int t2 = tile / P.tiles_w;
        const int th = t2 % P.tiles_h;
        n = t2 / P.tiles_h;
        oh0 = th * G::OH; ow0 = tw * G::OW;
    } else {                      // a pair of whole images
        n = tile * 2; oh0 = 0; ow0 = 0;
    }
    const int co0 = ctile * 32;
    // this workgroup's 8-channel chunks [c_lo, nchunks): nchunks is the END of the range.  GEO 0: even bounds (host); GEO 1: whole chunk pairs
    // spread as evenly as possible (w6_piece_bounds), the same bounds wherever the host's rule holds
    int c_lo, nchunks;
    if constexpr (GEO == 1) {
        w6_piece_bounds(a.Cin >> 3, nsplit, ks, c_lo, nchunks);
    } else {
        c_lo = (int)((long)ks * (a.Cin >> 3) / a.ksplit);
        nchunks = (int)((long)(ks + 1) * (a.Cin >> 3) / a.ksplit);
    }

    // ---- pass 1 item of this thread ----------------------------------------------------------------------------------------------
    // PAIR: thread = (item tid / 2, channel pair p_h = tid % 2 of its quad); lanes 4k..4k+3 then load the 32 contiguous bytes of a column
    int p_img, p_q, p_t, p_col;
    bool p_active;
    G::item_of(PAIR ? (tid >> 1) : tid, p_img, p_q, p_t, p_col, p_active);
    const int p_h = PAIR ? (tid & 1) : 0;
    // buffer resource over the image this thread stages (GEO 1: wave-uniform, waves 0-1 the first image of the pair, waves 2-3 the second
    // — PAIR: waves 0-3, 4-7; an image index past the batch gets an empty resource: every load returns 0): {base, num_records = bytes of
    // the image, raw dword format}
    const int img_n = n + (GEO == 1 ? (PAIR ? (wid >> 2) : (wave >> 1)) : 0);
    // (the size is set behind the base: as an argument of buffer_rsrc the test is evaluated in front of the base's readfirstlanes, and the scalar
    // code of the RoI-pair kernels moves with it)
    i32x4 rsrc = buffer_rsrc(P.x + (long)min(img_n, P.N - 1) * H * W * a.x_cs, 0);
    rsrc.z = __builtin_amdgcn_readfirstlane(img_n < P.N ? H * W * a.x_cs * 4 : 0);
    const int row_bytes = W * a.x_cs * 4;
    const int ih0 = oh0 - 1 + 4 * p_t, iw = ow0 - 1 + p_col;
    // byte offset of input row 0 of the item; rows above/below the image are out of the resource's range by themselves, a column
    // outside the image would alias the neighbouring row, so it is pushed out of range
    const int voff0 = (iw >= 0 && iw < W) ? (ih0 * W + iw) * a.x_cs * 4 + (a.x_co + p_q * 4 + p_h * 2) * 4 : (int)0x80000000;
    unsigned okm = 0;                                              // AFF only: relu(0*s + b) != 0, so padding needs the mask
    if (AFF) {
#pragma unroll
        for (int i = 0; i < 6; ++i) okm |= ((iw >= 0 && iw < W && ih0 + i >= 0 && ih0 + i < H) ? 1u : 0u) << i;
    }
    // scale/shift of the fused input affine: wave-uniform base (per chunk) + one 32-bit lane offset (two 64-bit lane pointers cost the
    // variant the registers it does not have)
    const unsigned aff_off = AFF ? (unsigned)(min(n + p_img, P.N - 1) * a.Cin + p_q * 4 + p_h * 2) : 0u;
    const f32x2 five = {5.0f, 5.0f};                   // the one transform coefficient that is not an inline constant: an SGPR pair
    // the thread's halo samples: 4 channels (a quad), PAIR 2 (a pair)
    using DV = std::conditional_t<PAIR, f32x2, f32x4>;
    DV d[6];
    DV in_sc, in_sh;
    if constexpr (PAIR) { in_sc = f32x2{1.f, 1.f}; in_sh = f32x2{0.f, 0.f}; }
    else { in_sc = f32x4{1.f, 1.f, 1.f, 1.f}; in_sh = f32x4{0.f, 0.f, 0.f, 0.f}; }
    auto load_D = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if constexpr (PAIR) d[i] = buffer_load_f32x2(rsrc, voff0 + i * row_bytes, chunk * 32, 0);
            else d[i] = buffer_load_f32x4(rsrc, voff0 + i * row_bytes, chunk * 32, 0);
        }
        if (AFF) {
            in_sc = *reinterpret_cast<const DV*>(P.in_scale + chunk * 8 + aff_off);
            in_sh = *reinterpret_cast<const DV*>(P.in_shift + chunk * 8 + aff_off);
        }
    };
    const int p_dst = w6_slot<GEO>(p_q, (GEO == 1 ? 4 * p_img : 0) + p_t, 0, p_col);
    auto pass1 = [&](f32x4* wbuf) {
        if (AFF) {
            // relu(x * s + b), and 0 for a sample outside the image (relu(0 * s + b) != 0): 2 packed fma per row, then ONE med3 per value —
            // med3(v, 0, +inf) = max(v, 0), med3(v, 0, 0) = 0 — with the row's third operand made from the mask bit
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const float kinf = ((okm >> i) & 1u) ? __builtin_inff() : 0.f;
                const DV v = __builtin_elementwise_fma(d[i], in_sc, in_sh);
                if constexpr (PAIR) d[i] = f32x2{__builtin_amdgcn_fmed3f(v.x, 0.f, kinf), __builtin_amdgcn_fmed3f(v.y, 0.f, kinf)};
                else d[i] = f32x4{__builtin_amdgcn_fmed3f(v.x, 0.f, kinf), __builtin_amdgcn_fmed3f(v.y, 0.f, kinf),
                                  __builtin_amdgcn_fmed3f(v.z, 0.f, kinf), __builtin_amdgcn_fmed3f(v.w, 0.f, kinf)};
            }
        }
        f32x2* dst = reinterpret_cast<f32x2*>(wbuf + p_dst) + p_h;
        if (GEO == 1 && !p_active) return;
#pragma unroll
        for (int h = 0; h < (PAIR ? 1 : 2); ++h) {    // channel pairs: 12 packed instructions and 6 ds_write_b64 each
            f32x2 e[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                if constexpr (PAIR) e[i] = d[i];
                else e[i] = h ? f32x2{d[i].z, d[i].w} : f32x2{d[i].x, d[i].y};
            }
            f32x2 w0, w1, w2, w3, w4, w5;
            w6_half_first(e[0], e[1], e[2], e[3], e[4], five, w0, w1, w2);
            w6_half_second(e[1], e[2], e[3], e[4], e[5], five, w3, w4, w5);
            dst[0 * 2 * W6_AP + h] = w0; dst[1 * 2 * W6_AP + h] = w1; dst[2 * 2 * W6_AP + h] = w2;
            dst[3 * 2 * W6_AP + h] = w3; dst[4 * 2 * W6_AP + h] = w4; dst[5 * 2 * W6_AP + h] = w5;
        }
    };

    // ---- MFMA side -------------------------------------------------------------------------------------------------------------
    // A operand row li = tile m (GEO 0: m = 10*t + tc, rows 30, 31 carry no tile and their accumulator rows are never stored); lane half hh = channel quad; accumulator register r of lane half hh is tile m = (r & 3) + 8*(r >> 2) + 4*hh, column
    // li = output channel co0 + li
    const int rowA = wave, rowB = 4 + (wave >> 1), halfB = wave & 1;
    int m_img, m_t, m_tc;
    G::tile_of(min(li, G::TILES - 1), m_img, m_t, m_tc);     // GEO 0: rows 30, 31 carry no tile; they re-read tile 29's samples (never stored)
    const f32x4* wl = sW + w6_slot<GEO>(hh, (GEO == 1 ? 4 * m_img : 0) + m_t, 0, 4 * m_tc);
    const f32x4* wA = wl + rowA * W6_AP;
    const f32x4* wB = wl + rowB * W6_AP;
    const f32x4* wBa = wB + (halfB ? G::CK : 0);                // see rdB
    const f32x4* wB3 = wB + (halfB ? 1 : 3 * G::CK);
    // U image: [chunk][cout tile][wave][9 slots][lane 64][4 floats]; slot k < 6: frequency (rowA, k); k >= 6: (rowB, 3*halfB + k - 6);
    // lane = 32*hh + li holds channels 8*chunk + 4*hh .. +3 of output channel 32*tile + li
    const float* u_wave = P.w + ((long)ct * 4 + wave) * (9 * 256);       // wave-uniform: the loads take it as a scalar base, lane * 16 B as offset
    const long u_chunk = (long)a.grid_y * (36 * 256);
    const int u_lane_off = lane * 4;
    f32x4 ub[3][3];
    auto load_U = [&](int step, int buf) {          // step = chunk*3 + s
        const int c = step / 3, s = step - c * 3;
        const float* src = u_wave + c * u_chunk + s * (3 * 256);
#pragma unroll
        for (int k = 0; k < 3; ++k) ub[buf][k] = *reinterpret_cast<const f32x4*>(src + (u_lane_off + k * 256));
    };
    const int total_steps = nchunks * 3;                        // END of the step range

    if (GEO == 1) {
        // halo columns 15..17 (image columns >= 14) are zero for every image this geometry accepts: their W slots are cleared here, once,
        // in both buffers, and pass 1 never touches them
        for (int i = tid; i < 2 * 2 * G::RG * 6 * 3; i += NT) {
            const int c3 = i % 3, rest = i / 3;
            const int a6 = rest % 6, r2 = rest / 6;
            const int r = r2 % G::RG, qb = r2 / G::RG;          // qb = buffer * 2 + quad
            sW[(qb >> 1) * G::WB + w6_slot<GEO>(qb & 1, r, a6, 15 + c3)] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    // ---- prologue ----------------------------------------------------------------------------------------------------------------
    // the halos of chunks 0 and 1 and the first weights are requested together: one memory round trip before the first MFMA
    load_D(c_lo);
    DV d_first[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) d_first[i] = d[i];
    DV sc_first = in_sc, sh_first = in_sh;
    load_D(min(c_lo + 1, nchunks - 1));
    load_U(c_lo * 3, 0);
    load_U(min(c_lo * 3 + 1, total_steps - 1), 1);
    {
        DV d_keep[6], sc_keep = in_sc, sh_keep = in_sh;
#pragma unroll
        for (int i = 0; i < 6; ++i) { d_keep[i] = d[i]; d[i] = d_first[i]; }
        in_sc = sc_first; in_sh = sh_first;
        pass1(sW);
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = d_keep[i];
        in_sc = sc_keep; in_sh = sh_keep;
    }

    f32x16 acc[9];
#pragma unroll
    for (int f = 0; f < 9; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[f][r] = 0.f;

    // ---- main loop: one period per 8-channel chunk ------------------------------------------------------------------------------
    //   barrier: W(c) complete, everybody is done with W(c-1)
    //   step 0 (row A, first half); pass 1 of chunk c+1 (in registers since the last period) into the other W buffer; request chunk c+2
    //   steps 1, 2 (row A second half, row B half)
    // The wave's 4 channels are transformed and consumed two at a time, which halves the live registers of pass 2.
    struct X5 { f32x2 x0, x1, x2, x3, x4; };
    // the five W samples one half of a frequency row needs, for channel pair h of the lane's quad: first half = columns 0..4 of the
    // tile's six, second half = columns 1..5 (slot offsets of w6_slot: +12 per column, column 4 -> +1, column 5 -> +13)
    auto rd = [&](const f32x4* wrow, bool second, int h) {
        const f32x2* w2 = reinterpret_cast<const f32x2*>(wrow) + h;
        X5 x;
        constexpr int K = G::CK;
        if (!second) { x.x0 = w2[0 * 2]; x.x1 = w2[K * 2]; x.x2 = w2[2 * K * 2]; x.x3 = w2[3 * K * 2]; x.x4 = w2[1 * 2]; }
        else         { x.x0 = w2[K * 2]; x.x1 = w2[2 * K * 2]; x.x2 = w2[3 * K * 2]; x.x3 = w2[1 * 2]; x.x4 = w2[(K + 1) * 2]; }
        return x;
    };
    // row B: which half is wave-uniform.  With A = row + (second half ? K : 0) both halves read A[0], A[K], A[2K], A[1] and one more sample,
    // A[3K] or A[1-K]: two address registers set up once (a branch between the two offset sets cost 22 VALU instructions per period in
    // address arithmetic and moves, each of which takes a slot from the matrix pipe)
    auto rdB = [&](const f32x4* wa, const f32x4* w3, int h) {
        const f32x2* a2 = reinterpret_cast<const f32x2*>(wa) + h;
        X5 x;
        constexpr int K = G::CK;
        x.x0 = a2[0]; x.x1 = a2[K * 2]; x.x2 = a2[2 * K * 2]; x.x3 = reinterpret_cast<const f32x2*>(w3)[h]; x.x4 = a2[1 * 2];
        return x;
    };
    auto mm = [&](const f32x2 v0, const f32x2 v1, const f32x2 v2, int h, int sbuf, int abase) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            acc[abase + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[s], ub[sbuf][0][2 * h + s], acc[abase + 0], 0, 0, 0);
            acc[abase + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[s], ub[sbuf][1][2 * h + s], acc[abase + 1], 0, 0, 0);
            acc[abase + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(v2[s], ub[sbuf][2][2 * h + s], acc[abase + 2], 0, 0, 0);
        }
    };
    // one half-step = 6 MFMAs: transform the samples read during the previous half-step, issue the MFMAs
    auto half_step = [&](const X5& x, bool second, int h, int sbuf, int abase) {
        f32x2 v0, v1, v2;
        if (!second) w6_half_first(x.x0, x.x1, x.x2, x.x3, x.x4, five, v0, v1, v2);
        else w6_half_second(x.x0, x.x1, x.x2, x.x3, x.x4, five, v0, v1, v2);
        mm(v0, v1, v2, h, sbuf, abase);
    };
    auto half_stepB = [&](const X5& x, int h) {      // MFMAs stay outside the branch: on both sides of one the allocator keeps two
        f32x2 v0, v1, v2;                           // copies of the accumulators they touch
        if (halfB == 0) { asm volatile("" ::: "memory"); w6_half_first(x.x0, x.x1, x.x2, x.x3, x.x4, five, v0, v1, v2); }
        else            { asm volatile("" ::: "memory"); w6_half_second(x.x0, x.x1, x.x2, x.x3, x.x4, five, v0, v1, v2); }
        mm(v0, v1, v2, h, 2, 6);
    };
    // two periods per trip: the W buffer of a period is then a compile-time offset of every LDS instruction (the parity as a register cost
    // vector adds per period)
    auto period = [&](const int c, auto parity) {
        constexpr int wcur = decltype(parity)::value * W6_WB;
        f32x4* wnext = sW + (1 - decltype(parity)::value) * W6_WB;
        const int step = c * 3;
        __syncthreads();
        // AHEAD (variants without the fused input affine): the LDS reads of half-step k+1 are issued in front of the MFMAs of half-step k.
        // With the affine its scale/shift registers leave no room for the second sample set (6 spilled registers, reloaded every period):
        // there each half-step reads its own samples.
        constexpr bool AHEAD = !AFF || PAIR;
        load_U(min(step + 2, total_steps - 1), 2);
        X5 xa = rd(wA + wcur, false, 0), xb;
        if (AHEAD) xb = rd(wA + wcur, false, 1);
        half_step(xa, false, 0, 0, 0);
        if (AHEAD) xa = rd(wA + wcur, true, 0); else xb = rd(wA + wcur, false, 1);
        half_step(xb, false, 1, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        pass1(wnext);
        load_D(min(c + 2, nchunks - 1));
        __builtin_amdgcn_sched_barrier(0);
        load_U(min(step + 3, total_steps - 1), 0);
        if (AHEAD) xb = rd(wA + wcur, true, 1); else xa = rd(wA + wcur, true, 0);
        half_step(xa, true, 0, 1, 3);
        if (AHEAD) xa = rdB(wBa + wcur, wB3 + wcur, 0); else xb = rd(wA + wcur, true, 1);
        half_step(xb, true, 1, 1, 3);
        __builtin_amdgcn_sched_barrier(0);
        load_U(min(step + 4, total_steps - 1), 1);
        if (AHEAD) xb = rdB(wBa + wcur, wB3 + wcur, 1); else xa = rdB(wBa + wcur, wB3 + wcur, 0);
        half_stepB(xa, 0);
        if (!AHEAD) xb = rdB(wBa + wcur, wB3 + wcur, 1);
        half_stepB(xb, 1);
    };
    for (int c = c_lo; c < nchunks; c += 2) {     // an even number of chunks: Cin is a multiple of 16 (validate), split-K bounds are even (host)
        period(c, std::integral_constant<int, 0>{});
        period(c + 1, std::integral_constant<int, 1>{});
    }

    // ---- epilogue (w6_epilogue, wino6_common.hpp) -----------------------------------------------------------------------------------
    // split-K: raw partial sums (no scale / shift / ReLU) go to slab ks of a.ws, whose first image is n_ws; the reduce kernel (conv.hip)
    // sums the slabs in a fixed order and applies the epilogue
    const W6Out<bool> out{nsplit > 1, ks, n_ws};
    // exchange area: 64 KiB from the start of LDS (PAIR: per half)
    w6_epilogue<GEO>(a, P, acc, smem, half * W6_EX_FLOATS, wave, lane, li, hh, std::true_type{}, co0, H, W, n, oh0, ow0, bx, out);
}

template <bool AFF, int GEO>
__global__ __launch_bounds__(256, 2) void conv_wino6_kernel(const ConvArgs a) {
    conv_wino6_body<AFF, GEO, false>(a);
}

// the paired form: 8 waves, one workgroup per CU (two waves per SIMD: the register budget of a conv_wino6 wave)
template <bool AFF, int GEO>
__global__ __launch_bounds__(512, 2) void conv_wino6p_kernel(const ConvArgs a) {
    conv_wino6_body<AFF, GEO, true>(a);
}

template <int GEO, bool PAIR>
static int launch_wino6_geo(ConvArgs& a, hipStream_t st, LaunchPlan* plan) {
    static DeviceOnce once;
    const auto k_plain = PAIR ? conv_wino6p_kernel<false, GEO> : conv_wino6_kernel<false, GEO>;
    const auto k_aff = PAIR ? conv_wino6p_kernel<true, GEO> : conv_wino6_kernel<true, GEO>;
    constexpr int lds = w6_lds_bytes<GEO, PAIR>();
    int rc = plan ? CMK_OK : once.run([&]() {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_plain), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_aff), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        return e == hipSuccess ? CMK_OK : fail(CMK_ELAUNCH, "conv_wino6: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    });
    if (rc) return rc;
    const int blocks = w6_assign_tiles<GEO>(a);
    a.grid_y = cdiv(a.Cout, 32);          // 32-cout tiles (the packed weights' layout); PAIR: the grid walks pairs of them
    a.total_tiles = blocks;
    if (a.ksplit < 1) a.ksplit = 1;
    const int gy = PAIR ? cdiv(a.grid_y, 2) : a.grid_y;
    if (GEO == 1 && a.ksplit > 1) {       // split-K of a whole RoI launch is the tail that takes every tile
        a.tail_tiles = blocks; a.tail_ksplit = a.ksplit; a.ksplit = 1;
    }
    if (GEO == 0 || a.tail_ksplit <= 1 || a.tail_tiles <= 0) a.tail_tiles = a.tail_ksplit = 0;
    if (a.tail_tiles > blocks) a.tail_tiles = blocks;
    a.main_blocks = ((blocks - a.tail_tiles + 7) / 8) * 8 * gy;
    // (the paired form runs two cout tiles per workgroup, the idle half of an odd last pair on the last tile's weights)
    if (plan) return w6_plan<GEO>(plan, a, PAIR ? "conv_wino6p_kernel" : "conv_wino6_kernel", blocks, PAIR ? 2 * gy : a.grid_y);
    const dim3 grid(a.main_blocks + ((a.tail_tiles + 7) / 8) * 8 * gy * a.tail_ksplit, a.ksplit);
    if constexpr (PAIR) {
        if (a.p[0].in_scale) hipLaunchKernelGGL((conv_wino6p_kernel<true, GEO>), grid, dim3(512), lds, st, a);
        else hipLaunchKernelGGL((conv_wino6p_kernel<false, GEO>), grid, dim3(512), lds, st, a);
    } else {
        if (a.p[0].in_scale) hipLaunchKernelGGL((conv_wino6_kernel<true, GEO>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((conv_wino6_kernel<false, GEO>), grid, dim3(256), lds, st, a);
    }
    return check_launch(PAIR ? "conv_wino6p" : "conv_wino6");
}

// geo 0: 12x40-pixel tiles of one image; geo 1: pairs of whole maps of at most 16 rows x 14 columns (one problem, no fused GN statistics);
// pair: the paired form (64 couts per workgroup)
int wino6_gn_records(int H, int W) { return W6_GN_RECS * cdiv(H, W6G<0>::OH) * cdiv(W, W6G<0>::OW); }

int launch_wino6(ConvArgs& a, int geo, bool pair, hipStream_t st, LaunchPlan* plan) {
    // (a split-K or tail workgroup stores with pixel stride cout_pad)
    if (int rc = w6_refuse_size(a, geo, std::max(a.y_cs, a.cout_pad), "conv_wino6")) return rc;
    // split-K of the map geometry keeps its even-split rule; the RoI-pair geometry gives every piece whole chunk pairs (w6_piece_bounds), so
    // there any number of ways up to the pair count goes
    if (a.ksplit > 1 && (a.nprob != 1 || a.gn_ws || !a.ws || (geo == 0 ? ((a.Cin >> 3) % (2 * a.ksplit)) != 0 : a.ksplit > (a.Cin >> 4)) ||
                         a.cout_pad < cdiv(a.Cout, 32) * 32))
        return fail(CMK_EINVAL, "conv_wino6: split-K takes one problem, no GroupNorm statistics, a workspace and Cin / 8 chunks %% (2 * splitk) == 0 (RoI pairs: splitk <= Cin / 16)%s", "");
    if (a.tail_ksplit > 1 && a.tail_tiles > 0) {
        if (geo != 1) return fail(CMK_EINVAL, "conv_wino6: tail split-K is a feature of the RoI-pair geometry (tune_wn 2)%s", "");
        if (a.ksplit > 1 || a.nprob != 1 || a.gn_ws || !a.ws || a.tail_ksplit > (a.Cin >> 4) || a.cout_pad < cdiv(a.Cout, 32) * 32)
            return fail(CMK_EINVAL, "conv_wino6: tail split-K takes one problem, no GroupNorm statistics, no split-K beside it, a workspace and at most Cin / 16 ways%s", "");
    }
    if (geo == 0) return pair ? launch_wino6_geo<0, true>(a, st, plan) : launch_wino6_geo<0, false>(a, st, plan);
    if (int rc = w6_refuse_roi_pairs(a, "conv_wino6: the RoI-pair geometry (with split-K or a split-K tail as without)")) return rc;
    return pair ? launch_wino6_geo<1, true>(a, st, plan) : launch_wino6_geo<1, false>(a, st, plan);
}

}  // namespace cmk

// Which tiles of a RoI-pair launch to split, and how many ways (cmk.h).  spatial_tiles x cout_tiles workgroups run on `slots` places at a
// time; the last, ragged round leaves most of the chip idle for a whole workgroup life.  Its whole spatial tiles become the tail.
extern "C" int cmk_wino6_tail_plan(int spatial_tiles, int cout_tiles, int chunk_pairs, int slots, int* tail_tiles, int* ways) {
    if (!tail_tiles || !ways) return CMK_EINVAL;
    *tail_tiles = *ways = 0;
    if (spatial_tiles <= 0 || cout_tiles <= 0 || slots <= 0) return CMK_OK;
    const long units = (long)spatial_tiles * cout_tiles;
    if (units < slots) return CMK_OK;                          // under one round: ordinary split-K territory
    const int tail_units = (int)(units % slots);
    if (tail_units == 0 || 2 * tail_units > slots) return CMK_OK;   // no ragged round, or one that fills over half the chip as it is
    const int tt = tail_units / cout_tiles;                    // whole spatial tiles
    if (tt == 0) return CMK_OK;
    for (int w = 8; w >= 2; w >>= 1)
        if ((long)tt * cout_tiles * w <= slots && w <= chunk_pairs) {
            *tail_tiles = tt; *ways = w;
            break;
        }
    return CMK_OK;
}

extern "C" void cmk_wino6_piece_bounds(int chunks, int ways, int piece, int* c_lo, int* c_hi) {
    cmk::w6_piece_bounds(chunks, ways, piece, *c_lo, *c_hi);
}

extern "C" int64_t cmk_wino6_packed_floats(int Cout, int Cin) {
    return (int64_t)((Cin + 7) / 8) * ((Cout + 31) / 32) * 36 * 256;
}
